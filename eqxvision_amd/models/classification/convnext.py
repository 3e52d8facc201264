"""ConvNeXt (reference models/classification/convnext.py:16-330).

Same fields / constructors / errors.  Device lowering of one block in inference (reference :62-72,
`x + layer_scale * block(x)`), see ops.cnblock:
  * C = 96 / 192 / 384 (the fused MLP kernels' widths): 7x7 depthwise conv (mv_cnblock_dw_fwd, normalize = 0) ->
    LayerNorm + fc1 + GELU + fc2 + layer_scale + residual (mv_ln_mlp_res_fwd / mv_ln_mlp_stream_res_fwd): 2 launches;
  * other widths: 7x7 depthwise conv + LayerNorm (normalize = 1) -> fc1 + GELU (LayerNorm affine folded) -> fc2 (layer_scale
    folded, fp32 residual in the epilogue): 3 launches;
  * fp32 mode, training mode, the switches off or shapes without a kernel: the composition of the generic entries.
The residual stream is fp32 NHWC from the stem (ops.patch4_ln) to the head, as in Swin.
"""
from __future__ import annotations

from functools import partial
from typing import Any, Callable, List, Optional, Sequence

import numpy as np

from ... import nn, ops
from ... import random as jr
from ..._act import head_fp32, residual_fp32
from ..._module import Module
from ...layers import ConvNormActivation, DropPath, LayerNorm2d, Linear2d
from ...nn import boundary
from ...utils import CLASSIFICATION_URLS, load_torch_weights


class CNBlock(Module):
    layer_scale: np.ndarray
    block: nn.Sequential
    stochastic_depth: DropPath

    def __init__(self, dim, layer_scale: float, stochastic_depth_prob: float,
                 norm_layer: Optional[Callable[..., Module]] = LayerNorm2d, *, key=None) -> None:
        if norm_layer is None:                                         # reference :28-29
            norm_layer = partial(nn.LayerNorm, eps=1e-6)
        keys = jr.split(key if key is not None else jr.PRNGKey(0), 4)
        self.block = nn.Sequential([
            nn.Conv2d(dim, dim, kernel_size=7, padding=3, groups=dim, use_bias=True, key=keys[0]),
            norm_layer(dim),
            Linear2d(in_features=dim, out_features=4 * dim, use_bias=True, key=keys[1]),
            nn.Lambda(nn.gelu),                                        # jax.nn.gelu: the tanh form
            Linear2d(in_features=4 * dim, out_features=dim, use_bias=True, key=keys[2]),
        ])
        self.layer_scale = (np.ones((dim, 1, 1), np.float32) * np.float32(layer_scale)).astype(np.float32)
        self.stochastic_depth = DropPath(p=stochastic_depth_prob, mode="local")

    @boundary
    def __call__(self, x, *, key=None):                                # reference :62-72
        from ... import grad as _grad
        if _grad.active():
            # layer_scale is a parameter no hooked op differentiates: refuse rather than return a gradient without it
            raise NotImplementedError("CNBlock was launched inside filter_value_and_grad by an op without a backward "
                                      "(eqxvision_amd/grad.py lists what is differentiable)")
        x = ops.as_map(x)
        sd = self.stochastic_depth
        if sd.inference or sd.p == 0.0:
            return ops.cnblock(x, self)
        if key is None:
            raise RuntimeError("DropPath requires a key when running in non-deterministic mode. Did you mean to enable inference?")
        keys = jr.split(ops._batched_keys(key, x.t.shape[0]), 2)       # reference :68: block, path
        return ops.cnblock(x, self, drop=(sd, keys[1]))


class _CNBlockConfig:
    # Stores information listed at Section 3 of the ConvNeXt paper
    def __init__(self, input_channels: int, out_channels: Optional[int], num_layers: int) -> None:
        self.input_channels = input_channels
        self.out_channels = out_channels
        self.num_layers = num_layers

    def __repr__(self) -> str:
        s = self.__class__.__name__ + "("
        s += "input_channels={input_channels}"
        s += ", out_channels={out_channels}"
        s += ", num_layers={num_layers}"
        s += ")"
        return s.format(**self.__dict__)


class ConvNeXt(Module):
    """A simple port of `torchvision.models.convnext`."""

    features: nn.Sequential
    avgpool: nn.AdaptiveAvgPool2d
    classifier: nn.Sequential

    def __init__(self, block_setting: Sequence[_CNBlockConfig], stochastic_depth_prob: float = 0.0, layer_scale: float = 1e-6,
                 num_classes: int = 1000, block: Optional[Module] = None, norm_layer: Optional[Module] = None, *,
                 key=None) -> None:
        if not block_setting:                                          # reference :129-135
            raise ValueError("The block_setting should not be empty")
        elif not (isinstance(block_setting, Sequence) and all([isinstance(s, _CNBlockConfig) for s in block_setting])):
            raise TypeError("The block_setting should be List[CNBlockConfig]")
        if key is None:
            key = jr.PRNGKey(0)
        keys = jr.split(key, 2)
        if block is None:
            block = CNBlock
        if norm_layer is None:
            norm_layer = partial(LayerNorm2d, eps=1e-6)
        layers: List[Module] = []
        firstconv_output_channels = block_setting[0].input_channels
        layers.append(ConvNormActivation(in_channels=3, out_channels=firstconv_output_channels, kernel_size=4, stride=4, padding=0,
                                         norm_layer=norm_layer, activation_layer=None, use_bias=True, key=keys[0]))
        total_stage_blocks = sum(cnf.num_layers for cnf in block_setting)
        stage_block_id = 0
        for cnf in block_setting:
            stage: List[Module] = []
            for _ in range(cnf.num_layers):
                keys = jr.split(keys[1], 2)
                sd_prob = stochastic_depth_prob * stage_block_id / (total_stage_blocks - 1.0)     # reference :170-172
                stage.append(block(cnf.input_channels, layer_scale, sd_prob, key=keys[0]))
                stage_block_id += 1
            layers.append(nn.Sequential(stage))
            if cnf.out_channels is not None:
                keys = jr.split(keys[1], 2)
                layers.append(nn.Sequential([
                    norm_layer(cnf.input_channels),
                    nn.Conv2d(cnf.input_channels, cnf.out_channels, kernel_size=2, stride=2, key=keys[0]),
                ]))
        self.features = nn.Sequential(layers)
        self.avgpool = nn.AdaptiveAvgPool2d(1)
        lastblock = block_setting[-1]
        lastconv_output_channels = lastblock.out_channels if lastblock.out_channels is not None else lastblock.input_channels
        self.classifier = nn.Sequential([
            norm_layer(lastconv_output_channels),
            nn.Lambda(np.ravel),
            nn.Linear(lastconv_output_channels, num_classes, key=keys[1]),
        ])

    def _features(self, x, key=None):
        """self.features(x) with the fp32 residual stream: the stem (4x4/4 conv + LayerNorm2d) writes it in one launch, each
        downsample (LayerNorm2d + 2x2/2 conv, ops.convnext_downsample) returns to it.  `key`: split per layer like nn.Sequential does."""
        L = self.features.layers
        ks = [None] * len(L) if key is None else list(jr.split(key, len(L)))
        stem = L[0]
        if not (residual_fp32() and isinstance(stem, nn.Sequential) and len(stem) == 2 and type(stem.layers[0]) is nn.Conv2d
                and isinstance(stem.layers[1], nn.LayerNorm)):
            return self.features(x, key=key)
        y = ops.patch4_ln(x, stem.layers[0], stem.layers[1])
        if y is None:
            y = ops.conv2d_entry_split(x, stem.layers[0])
            y = y if y is not None else ops.conv2d(x, stem.layers[0])
            y = ops.layernorm(y, stem.layers[1], out_fp32=True)
        x = y
        for layer, k in zip(L[1:], ks[1:]):
            if (isinstance(layer, nn.Sequential) and len(layer) == 2 and isinstance(layer.layers[0], nn.LayerNorm)
                    and type(layer.layers[1]) is nn.Conv2d):
                x = ops.convnext_downsample(x, layer.layers[0], layer.layers[1])
            else:
                x = layer(x, key=k)
        return x

    @boundary
    def __call__(self, x, *, key=None):                                # reference :211-220
        x = self._features(x, key=key)
        norm = self.classifier.layers[0]
        if head_fp32() and isinstance(norm, nn.LayerNorm) and type(self.avgpool) is nn.AdaptiveAvgPool2d:
            x = ops.adaptive_avgpool2d(x, self.avgpool.target_shape, out_fp32=True)
            x = ops.layernorm(x, norm, out_fp32=True)
        else:
            x = self.avgpool(x)
            x = norm(x)
        x = ops.flatten(x)
        return ops.linear_head(x, self.classifier.layers[2])


def _convnext(arch: str, block_setting: List[_CNBlockConfig], stochastic_depth_prob: float, torch_weights: str,
              **kwargs: Any) -> ConvNeXt:
    model = ConvNeXt(block_setting, stochastic_depth_prob=stochastic_depth_prob, **kwargs)
    if torch_weights:
        if arch not in CLASSIFICATION_URLS:                            # reference :237-238
            raise ValueError(f"No checkpoint is available for model type {arch}")
        model = load_torch_weights(model, torch_weights=torch_weights)
    return model


def convnext_tiny(*, torch_weights: str = None, **kwargs: Any) -> ConvNeXt:
    """ConvNeXt Tiny (`A ConvNet for the 2020s`, https://arxiv.org/abs/2201.03545)."""
    block_setting = [_CNBlockConfig(96, 192, 3), _CNBlockConfig(192, 384, 3), _CNBlockConfig(384, 768, 9),
                     _CNBlockConfig(768, None, 3)]
    stochastic_depth_prob = kwargs.pop("stochastic_depth_prob", 0.1)
    return _convnext("convnext_tiny", block_setting, stochastic_depth_prob, torch_weights, **kwargs)


def convnext_small(*, torch_weights: str = None, **kwargs: Any) -> ConvNeXt:
    """ConvNeXt Small."""
    block_setting = [_CNBlockConfig(96, 192, 3), _CNBlockConfig(192, 384, 3), _CNBlockConfig(384, 768, 27),
                     _CNBlockConfig(768, None, 3)]
    stochastic_depth_prob = kwargs.pop("stochastic_depth_prob", 0.4)
    return _convnext("convnext_small", block_setting, stochastic_depth_prob, torch_weights, **kwargs)


def convnext_base(*, torch_weights: str = None, **kwargs: Any) -> ConvNeXt:
    """ConvNeXt Base."""
    block_setting = [_CNBlockConfig(128, 256, 3), _CNBlockConfig(256, 512, 3), _CNBlockConfig(512, 1024, 27),
                     _CNBlockConfig(1024, None, 3)]
    stochastic_depth_prob = kwargs.pop("stochastic_depth_prob", 0.5)
    return _convnext("convnext_base", block_setting, stochastic_depth_prob, torch_weights, **kwargs)


def convnext_large(*, torch_weights: str = None, **kwargs: Any) -> ConvNeXt:
    """ConvNeXt Large."""
    block_setting = [_CNBlockConfig(192, 384, 3), _CNBlockConfig(384, 768, 3), _CNBlockConfig(768, 1536, 27),
                     _CNBlockConfig(1536, None, 3)]
    stochastic_depth_prob = kwargs.pop("stochastic_depth_prob", 0.5)
    return _convnext("convnext_large", block_setting, stochastic_depth_prob, torch_weights, **kwargs)
