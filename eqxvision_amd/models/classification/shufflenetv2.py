"""ShuffleNetV2 x0.5 / x1.0 / x1.5 / x2.0 (reference models/classification/shufflenetv2.py:16-331).

Same fields / constructors / errors.  Device lowering of one unit in bf16 inference (reference :104-112, `concatenate` ->
`_channel_shuffle`), see ops.shuffle_unit:
  * every unit output is ONE tensor [B, H, W, 2P] in the folded layout (P = the branch width rounded up to 8; left half at channel 0,
    right half at channel P, exact zeros at the pads).  The shuffle, the split and the concatenation are permutations of channels in
    front of a convolution, i.e. permutations of the next unit's weight columns: none of them is ever launched;
  * stride 1: the first 1x1 of branch2 (mv_conv2d_nhwc_fwd over the whole physical tensor, columns permuted) -> depthwise 3x3 + BN ->
    1x1 + BN + relu AND the pass-through half in one launch (mv_shuffle_dwpw_fwd): 2 launches;
  * stride 2: branch1's depthwise + 1x1 (mv_shuffle_dwpw_fwd), branch2's first 1x1, branch2's depthwise + 1x1: 3 launches;
  * conv5 reads the folded tensor through permuted weight columns; pool and fc as in ResNet;
  * fp32 mode, training-mode BatchNorm, the switches ("no_shuffle_dwpw", "force_generic") or shapes without a kernel: the literal
    composition on logical channels (split by mv_copy_rows, ops.conv2d, ops.concat_channels, one mv_channel_gather_nhwc_fwd for the
    shuffle).
"""
from __future__ import annotations

from typing import Any, List

import numpy as np

from ... import nn, ops
from ... import random as jr
from ..._act import head_fp32
from ..._module import Module
from ...nn import boundary
from ...utils import load_torch_weights


def _refuse_grad():
    from ... import grad as _grad
    if _grad.active():
        # the folded kernels and the channel gather have no backward: refuse rather than return a gradient without them
        raise NotImplementedError("ShuffleNetV2's _InvertedResidual was launched inside filter_value_and_grad by an op without a "
                                  "backward (eqxvision_amd/grad.py lists what is differentiable)")


def _channel_shuffle(x, groups: int):
    """reference :16-23: (groups, C / groups) -> (C / groups, groups) over the channel axis, as one gather."""
    x = ops.as_map(x)
    C = x.t.shape[-1]
    j = np.arange(C)
    idx = (j % groups) * (C // groups) + j // groups
    return ops.channel_gather(x, ops._dev(idx.astype(np.int32), ops.torch.int32))


class _InvertedResidual(Module):
    stride: int
    branch1: nn.Sequential
    branch2: nn.Sequential

    def __init__(self, inp: int, oup: int, stride: int, *, key=None) -> None:
        keys = jr.split(key if key is not None else jr.PRNGKey(0), 5)
        if not (1 <= stride <= 3):                                     # reference :41-42
            raise ValueError("illegal stride value")
        branch_features = oup // 2
        assert (stride != 1) or (inp == branch_features << 1)          # reference :45
        self.stride = stride
        if stride > 1:
            self.branch1 = nn.Sequential([
                self.depthwise_conv(inp, inp, kernel_size=3, stride=self.stride, padding=1, key=keys[0]),
                nn.BatchNorm(inp, axis_name="batch"),
                nn.Conv2d(inp, branch_features, kernel_size=1, stride=1, padding=0, use_bias=False, key=keys[1]),
                nn.BatchNorm(branch_features, axis_name="batch"),
                nn.Lambda(nn.relu),
            ])
        else:
            self.branch1 = nn.Sequential([nn.Identity()])              # reference :72: no parameters
        self.branch2 = nn.Sequential([
            nn.Conv2d(inp if (self.stride > 1) else branch_features, branch_features, kernel_size=1, stride=1, padding=0,
                      use_bias=False, key=keys[2]),
            nn.BatchNorm(branch_features, axis_name="batch"),
            nn.Lambda(nn.relu),
            self.depthwise_conv(branch_features, branch_features, kernel_size=3, stride=self.stride, padding=1, key=keys[3]),
            nn.BatchNorm(branch_features, axis_name="batch"),
            nn.Conv2d(branch_features, branch_features, kernel_size=1, stride=1, padding=0, use_bias=False, key=keys[4]),
            nn.BatchNorm(branch_features, axis_name="batch"),
            nn.Lambda(nn.relu),
        ])

    @staticmethod
    def depthwise_conv(i: int, o: int, kernel_size: int, stride: int = 1, padding: int = 0, bias: bool = False, key=None) -> nn.Conv2d:
        return nn.Conv2d(i, o, kernel_size, stride, padding, use_bias=bias, groups=i, key=key)

    @boundary
    def __call__(self, x, *, key=None):                                # reference :104-112
        _refuse_grad()
        # a unit called on its own takes and returns LOGICAL channels; inside ShuffleNetV2 the folded layout travels from unit to unit
        y, layout = ops.shuffle_unit(ops.as_map(x), self, None)
        return ops.shuffle_unfold(y, layout, self)


class ShuffleNetV2(Module):
    """A simple port of `torchvision.models.shufflenetv2`."""

    conv1: nn.Sequential
    maxpool: nn.MaxPool2d
    stage2: nn.Sequential
    stage3: nn.Sequential
    stage4: nn.Sequential
    conv5: nn.Sequential
    pool: nn.AdaptiveAvgPool2d
    fc: nn.Linear

    def __init__(self, stages_repeats: List[int], stages_out_channels: List[int], num_classes: int = 1000,
                 inverted_residual: Module = _InvertedResidual, *, key=None) -> None:
        if key is None:
            key = jr.PRNGKey(0)
        keys = jr.split(key, 2)
        if len(stages_repeats) != 3:                                   # reference :154-157
            raise ValueError("expected stages_repeats as list of 3 positive ints")
        if len(stages_out_channels) != 5:
            raise ValueError("expected stages_out_channels as list of 5 positive ints")
        input_channels = 3
        output_channels = stages_out_channels[0]
        self.conv1 = nn.Sequential([
            nn.Conv2d(input_channels, output_channels, 3, 2, 1, use_bias=False, key=keys[0]),
            nn.BatchNorm(output_channels, axis_name="batch"),
            nn.Lambda(nn.relu),
        ])
        input_channels = output_channels
        self.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
        stage_names = [f"stage{i}" for i in [2, 3, 4]]
        for name, repeats, output_channels in zip(stage_names, stages_repeats, stages_out_channels[1:]):
            keys = jr.split(keys[1], 2)
            seq = [inverted_residual(input_channels, output_channels, 2, key=keys[0])]
            for i in range(repeats - 1):
                keys = jr.split(keys[1], 2)
                seq.append(inverted_residual(output_channels, output_channels, 1, key=keys[0]))
            setattr(self, name, nn.Sequential(seq))
            input_channels = output_channels
        keys = jr.split(keys[1], 2)
        output_channels = stages_out_channels[-1]
        self.conv5 = nn.Sequential([
            nn.Conv2d(input_channels, output_channels, 1, 1, 0, use_bias=False, key=keys[0]),
            nn.BatchNorm(output_channels, axis_name="batch"),
            nn.Lambda(nn.relu),
        ])
        self.pool = nn.AdaptiveAvgPool2d((1, 1))
        self.fc = nn.Linear(output_channels, num_classes, key=keys[1])

    def _units(self):
        """The units of the three stages in order when every one is the reference's _InvertedResidual, else None."""
        units = []
        for stage in (self.stage2, self.stage3, self.stage4):
            if not isinstance(stage, nn.Sequential):
                return None
            units += list(stage.layers)
        return units if all(type(u) is _InvertedResidual for u in units) else None

    @boundary
    def __call__(self, x, *, key=None):                                # reference :215-230 (no layer of this family consumes a key)
        _refuse_grad()
        L1 = self.conv1.layers
        if len(L1) == 3 and type(L1[0]) is nn.Conv2d and isinstance(L1[1], nn.BatchNorm) and isinstance(L1[2], nn.Lambda) \
                and nn.act_name(L1[2].fn) == "relu" and type(self.maxpool) is nn.MaxPool2d:
            x = ops.stem_conv_pool(x, L1[0], L1[1], "relu", self.maxpool)
        else:
            x = self.maxpool(self.conv1(x))
        units = self._units()
        L5 = self.conv5.layers
        if units is None or not (len(L5) == 3 and type(L5[0]) is nn.Conv2d and isinstance(L5[1], nn.BatchNorm)
                                 and isinstance(L5[2], nn.Lambda) and nn.act_name(L5[2].fn) == "relu"):
            x = self.conv5(self.stage4(self.stage3(self.stage2(x))))
        else:
            layout = None
            for u in units:                                            # the folded layout travels from unit to unit
                x, layout = ops.shuffle_unit(x, u, layout)
            x = ops.shuffle_head(x, L5[0], L5[1], layout)
        if type(self.pool) is nn.AdaptiveAvgPool2d and head_fp32():
            x = ops.adaptive_avgpool2d(x, self.pool.target_shape, out_fp32=True)
        else:
            x = self.pool(x)
        x = ops.flatten(x)
        return ops.linear_head(x, self.fc)


def _shufflenetv2(*args: Any, **kwargs: Any) -> ShuffleNetV2:
    return ShuffleNetV2(*args, **kwargs)


def shufflenet_v2_x0_5(torch_weights: str = None, **kwargs: Any) -> ShuffleNetV2:
    """ShuffleNetV2 with 0.5x output channels (`ShuffleNet V2: Practical Guidelines for Efficient CNN Architecture Design`,
    https://arxiv.org/abs/1807.11164)."""
    model = _shufflenetv2([4, 8, 4], [24, 48, 96, 192, 1024], **kwargs)
    if torch_weights:
        model = load_torch_weights(model, torch_weights=torch_weights)
    return model


def shufflenet_v2_x1_0(torch_weights: str = None, **kwargs: Any) -> ShuffleNetV2:
    """ShuffleNetV2 with 1.0x output channels."""
    model = _shufflenetv2([4, 8, 4], [24, 116, 232, 464, 1024], **kwargs)
    if torch_weights:
        model = load_torch_weights(model, torch_weights=torch_weights)
    return model


def shufflenet_v2_x1_5(torch_weights: str = None, **kwargs: Any) -> ShuffleNetV2:
    """ShuffleNetV2 with 1.5x output channels."""
    model = _shufflenetv2([4, 8, 4], [24, 176, 352, 704, 1024], **kwargs)
    if torch_weights:
        model = load_torch_weights(model, torch_weights=torch_weights)
    return model


def shufflenet_v2_x2_0(torch_weights: str = None, **kwargs: Any) -> ShuffleNetV2:
    """ShuffleNetV2 with 2.0x output channels."""
    model = _shufflenetv2([4, 8, 4], [24, 244, 488, 976, 2048], **kwargs)
    if torch_weights:
        model = load_torch_weights(model, torch_weights=torch_weights)
    return model
