"""SqueezeNet 1.0 / 1.1 (reference models/classification/squeezenet.py:14-172).

Same fields / constructors / defaults.  Device lowering of the bf16 forward:
  * the entry convolution + ReLU is one launch, every max pool is the ceil-mode pooling (mv_maxpool2d_out_nhwc_fwd);
  * a Fire module is 2 launches (ops.fire): the squeeze 1x1 + ReLU on the ordinary convolution path, then both expand convolutions,
    their ReLUs and the concatenation in one (mv_fire_expand_fwd: each half lands in its channel slice, nothing is copied);
  * the classifier: Dropout (the identity in inference; ops.dropout on the jax.random bit stream otherwise), the final 1x1
    convolution + ReLU in one launch, the global average in fp32, the flatten;
  * fp32 mode, the switches ("no_fire_expand", "force_generic") or shapes without a kernel: the literal composition (three
    convolutions + ops.concat_channels).
No backward: a Fire inside filter_value_and_grad refuses.
"""
from __future__ import annotations

from typing import Any, Optional

from ... import nn, ops
from ... import random as jr
from ..._act import head_fp32
from ..._module import Module
from ...nn import boundary
from ...utils import load_torch_weights


def _refuse_grad():
    from ... import grad as _grad
    if _grad.active():
        # the expand kernel, the concatenation and the ceil-mode pooling have no backward: refuse rather than return a gradient
        # without them
        raise NotImplementedError("SqueezeNet's _Fire was launched inside filter_value_and_grad by an op without a backward "
                                  "(eqxvision_amd/grad.py lists what is differentiable)")


class _Fire(Module):
    inplanes: int
    squeeze: nn.Conv2d
    squeeze_activation: nn.Lambda
    expand1x1: nn.Conv2d
    expand1x1_activation: nn.Lambda
    expand3x3: nn.Conv2d
    expand3x3_activation: nn.Lambda

    def __init__(self, inplanes: int, squeeze_planes: int, expand1x1_planes: int, expand3x3_planes: int, key=None) -> None:
        keys = jr.split(key if key is not None else jr.PRNGKey(0), 3)
        self.inplanes = inplanes
        self.squeeze = nn.Conv2d(inplanes, squeeze_planes, kernel_size=1, key=keys[0])
        self.squeeze_activation = nn.Lambda(nn.relu)
        self.expand1x1 = nn.Conv2d(squeeze_planes, expand1x1_planes, kernel_size=1, key=keys[1])
        self.expand1x1_activation = nn.Lambda(nn.relu)
        self.expand3x3 = nn.Conv2d(squeeze_planes, expand3x3_planes, kernel_size=3, padding=1, key=keys[2])
        self.expand3x3_activation = nn.Lambda(nn.relu)

    @boundary
    def __call__(self, x, *, key=None):                                # reference :45-53
        _refuse_grad()
        return ops.fire(ops.as_map(x), self)


_PLANS = {
    # (entry kernel, entry width), then Fire (inplanes, squeeze, expand1x1, expand3x3) or "pool"
    "1_0": ((7, 96), (96, 16, 64, 64), (128, 16, 64, 64), (128, 32, 128, 128), "pool", (256, 32, 128, 128), (256, 48, 192, 192),
            (384, 48, 192, 192), (384, 64, 256, 256), "pool", (512, 64, 256, 256)),
    "1_1": ((3, 64), (64, 16, 64, 64), (128, 16, 64, 64), "pool", (128, 32, 128, 128), (256, 32, 128, 128), "pool",
            (256, 48, 192, 192), (384, 48, 192, 192), (384, 64, 256, 256), (512, 64, 256, 256)),
}


class SqueezeNet(Module):
    """A simple port of `torchvision.models.squeezenet`."""

    features: nn.Sequential
    classifier: nn.Sequential

    def __init__(self, version: str = "1_0", num_classes: int = 1000, dropout: float = 0.5, *, key=None) -> None:
        if key is None:
            key = jr.PRNGKey(0)
        keys = jr.split(key, 10)
        plan = _PLANS.get(version)
        if plan is not None:                                           # reference :83-118: any other version leaves `features` unset
            (k, width), rest = plan[0], plan[1:]
            layers = [nn.Conv2d(3, width, kernel_size=k, stride=2, key=keys[0]), nn.Lambda(nn.relu),
                      nn.MaxPool2d(kernel_size=3, stride=2, use_ceil=True)]
            fire_keys = iter(keys[1:9])
            for item in rest:
                layers.append(nn.MaxPool2d(kernel_size=3, stride=2, use_ceil=True) if item == "pool"
                              else _Fire(*item, key=next(fire_keys)))
            self.features = nn.Sequential(layers)
        final_conv = nn.Conv2d(512, num_classes, kernel_size=1, key=keys[9])
        self.classifier = nn.Sequential([
            nn.Dropout(p=dropout),
            final_conv,
            nn.Lambda(nn.relu),
            nn.AdaptiveAvgPool2d((1, 1)),
        ])

    @boundary
    def __call__(self, x, *, key=None):                                # reference :131-139
        _refuse_grad()
        x = self.features(x)                                           # (the reference hands the features no key)
        L = self.classifier.layers
        if not (len(L) == 4 and isinstance(L[0], nn.Dropout) and type(L[1]) is nn.Conv2d and isinstance(L[2], nn.Lambda)
                and nn.act_name(L[2].fn) == "relu" and type(L[3]) is nn.AdaptiveAvgPool2d):
            return ops.flatten(self.classifier(x, key=key))
        drop, conv, _, pool = L
        if nn.dropout_live(drop):
            if key is None:
                raise RuntimeError("Dropout requires a key when running in non-deterministic mode.")
            x = ops.as_map(x)
            keys = jr.split(ops._batched_keys(key, x.t.shape[0]), len(L))      # nn.Sequential: one key per layer, Dropout is layer 0
            x = drop(x, key=keys[0])
        x = ops.conv2d(x, conv, None, "relu")
        x = ops.adaptive_avgpool2d(x, pool.target_shape, out_fp32=True) if head_fp32() else pool(x)
        return ops.flatten(x)


def _squeezenet(version: str, torch_weights: Optional[str], **kwargs: Any) -> SqueezeNet:
    model = SqueezeNet(version, **kwargs)
    if torch_weights:
        model = load_torch_weights(model, torch_weights=torch_weights)
    return model


def squeezenet1_0(torch_weights: str = None, **kwargs: Any) -> SqueezeNet:
    """SqueezeNet 1.0 (`SqueezeNet: AlexNet-level accuracy with 50x fewer parameters and <0.5MB model size`,
    https://arxiv.org/abs/1602.07360).  The minimum input size is 21 x 21."""
    return _squeezenet("1_0", torch_weights, **kwargs)


def squeezenet1_1(torch_weights: str = None, **kwargs: Any) -> SqueezeNet:
    """SqueezeNet 1.1 (https://github.com/DeepScale/SqueezeNet/tree/master/SqueezeNet_v1.1): 2.4x less computation and slightly
    fewer parameters than 1.0 at the same accuracy.  The minimum input size is 17 x 17."""
    return _squeezenet("1_1", torch_weights, **kwargs)
