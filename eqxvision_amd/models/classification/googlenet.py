"""GoogLeNet / Inception v1 (reference models/classification/googlenet.py:15-335).

Same fields / constructors / defaults.  Device lowering of the bf16 inference forward:
  * conv1 is the image-entry convolution, conv2 / conv3 the ordinary convolution with BatchNorm (eps 1e-3) folded, the four stage
    pools the ceil-mode pooling (mv_maxpool2d_out_nhwc_fwd);
  * an Inception module is 4 launches (ops.inception): the merged 1x1 of branch 1 and the two reduce convolutions
    (mv_conv1x1_split_fwd: branch 1 lands in its channel slice of the output), the stride-1 max pool, the pool projection into its
    slice, both 3x3 convolutions into theirs (mv_conv3x3_pair_fwd) -- nothing is concatenated;
  * the head: the global average in fp32, the flatten, Dropout (the identity in inference), the fp32 classifier; with
    `aux_logits=True` the two auxiliary heads run as well and the call returns (logits, aux2, aux1), as the reference does in
    inference too;
  * training mode (BatchNorm on batch statistics), fp32 mode, the switches ("no_inception_fused", "force_generic") or module shapes
    without a kernel: the literal composition (six convolutions, the pool and ops.concat_channels per module).
Branch 3 is a 3x3 convolution (torchvision's known "5x5" bug, kept by the reference).  The key schedule is the reference's: the forward
splits its key in 14 and jax clamps the out-of-range indices 14 and 15 to 13, so the main Dropout draws from element 13; an auxiliary
head splits elements 7 / 11 in two and its Dropout draws from the second.  No backward: the family refuses inside filter_value_and_grad.
"""
from __future__ import annotations

import warnings
from typing import Any, Callable, List, Optional

from ... import nn, ops
from ... import random as jr
from ..._act import head_fp32
from ..._module import Module, _rebuild
from ...nn import boundary
from ...utils import load_torch_weights


def _refuse_grad():
    from ... import grad as _grad
    if _grad.active():
        # the Inception kernels, the concatenation and the ceil-mode pooling have no backward: refuse rather than return a gradient
        # without them
        raise NotImplementedError("GoogLeNet was launched inside filter_value_and_grad by an op without a backward "
                                  "(eqxvision_amd/grad.py lists what is differentiable)")


class BasicConv2d(Module):
    conv: nn.Conv2d
    bn: nn.BatchNorm

    def __init__(self, in_channels: int, out_channels: int, *, key=None, **kwargs: Any) -> None:
        self.conv = nn.Conv2d(in_channels, out_channels, use_bias=False, key=key, **kwargs)
        self.bn = nn.BatchNorm(out_channels, axis_name="batch", eps=0.001)

    @boundary
    def __call__(self, x, *, key=None):                                # reference :305-310 (BatchNorm ignores the key)
        _refuse_grad()
        return ops.conv2d(x, self.conv, self.bn, "relu")


class _Inception(Module):
    branch1: Module
    branch2: nn.Sequential
    branch3: nn.Sequential
    branch4: nn.Sequential

    def __init__(self, in_channels: int, ch1x1: int, ch3x3red: int, ch3x3: int, ch5x5red: int, ch5x5: int, pool_proj: int,
                 conv_block: Optional[Callable[..., Module]] = None, *, key=None) -> None:
        if conv_block is None:
            conv_block = BasicConv2d
        keys = jr.split(key if key is not None else jr.PRNGKey(0), 5)
        self.branch1 = conv_block(in_channels, ch1x1, kernel_size=1, key=keys[0])
        self.branch2 = nn.Sequential([conv_block(in_channels, ch3x3red, kernel_size=1, key=keys[1]),
                                      conv_block(ch3x3red, ch3x3, kernel_size=3, padding=1, key=keys[2])])
        # kernel_size=3 instead of 5 is torchvision's known bug (pytorch/vision issue 906), kept by the reference
        self.branch3 = nn.Sequential([conv_block(in_channels, ch5x5red, kernel_size=1, key=keys[3]),
                                      conv_block(ch5x5red, ch5x5, kernel_size=3, padding=1, key=keys[4])])
        # (the reference indexes keys[5] of a 5-way split: jax clamps it to keys[4])
        self.branch4 = nn.Sequential([nn.MaxPool2d(kernel_size=3, stride=1, padding=1, use_ceil=True),
                                      conv_block(in_channels, pool_proj, kernel_size=1, key=keys[4])])

    @boundary
    def __call__(self, x, *, key=None):                                # reference :229-237
        _refuse_grad()
        return ops.inception(ops.as_map(x), self)


class InceptionAux(Module):
    conv: Module
    fc1: nn.Linear
    fc2: nn.Linear
    dropout: nn.Dropout
    avgpool: nn.AdaptiveAvgPool2d

    def __init__(self, in_channels: int, num_classes: int, conv_block: Optional[Callable[..., Module]] = None, dropout: float = 0.7,
                 *, key=None) -> None:
        if conv_block is None:
            conv_block = BasicConv2d
        keys = jr.split(key if key is not None else jr.PRNGKey(0), 3)
        self.conv = conv_block(in_channels, 128, kernel_size=1, key=keys[0])
        self.fc1 = nn.Linear(2048, 1024, key=keys[1])
        self.fc2 = nn.Linear(1024, num_classes, key=keys[2])
        self.dropout = nn.Dropout(p=dropout)
        self.avgpool = nn.AdaptiveAvgPool2d((4, 4))

    @boundary
    def __call__(self, x, *, key=None):                                # reference :268-284
        _refuse_grad()
        x = self.avgpool(ops.as_map(x))                                # 14 x 14 -> 4 x 4: unequal windows (equinox's bounds)
        x = self.conv(x)
        x = ops.flatten(x)                                             # jnp.ravel of the (C, H, W) sample
        x = ops.linear(x, self.fc1, "relu", out_fp32=head_fp32())    # a classifier head: fp32 from here on, like the main one
        if nn.dropout_live(self.dropout):
            if key is None:
                raise RuntimeError("Dropout requires a key when running in non-deterministic mode.")
            x = self.dropout(x, key=jr.split(ops._batched_keys(key, x.t.shape[0]), 2)[1])
        return ops.linear_head(x, self.fc2)


class GoogLeNet(Module):
    """A simple port of `torchvision.models.GoogLeNet`."""

    aux_logits: bool
    conv1: Module
    maxpool1: nn.MaxPool2d
    conv2: Module
    conv3: Module
    maxpool2: nn.MaxPool2d
    inception3a: Module
    inception3b: Module
    maxpool3: nn.MaxPool2d
    inception4a: Module
    inception4b: Module
    inception4c: Module
    inception4d: Module
    inception4e: Module
    maxpool4: nn.MaxPool2d
    inception5a: Module
    inception5b: Module
    aux1: Module
    aux2: Module
    avgpool: nn.AdaptiveAvgPool2d
    dropout: nn.Dropout
    fc: nn.Linear

    def __init__(self, num_classes: int = 1000, aux_logits: bool = False, blocks: Optional[List[Callable[..., Module]]] = None,
                 dropout: float = 0.2, dropout_aux: float = 0.7, *, key=None) -> None:
        if blocks is None:
            blocks = [BasicConv2d, _Inception, InceptionAux]
        assert len(blocks) == 3
        conv_block, inception_block, inception_aux_block = blocks
        if key is None:
            key = jr.PRNGKey(0)
        keys = jr.split(key, 20)

        self.aux_logits = aux_logits
        self.conv1 = conv_block(3, 64, kernel_size=7, stride=2, padding=3, key=keys[0])
        self.maxpool1 = nn.MaxPool2d(3, stride=2, use_ceil=True)
        self.conv2 = conv_block(64, 64, kernel_size=1, key=keys[1])
        self.conv3 = conv_block(64, 192, kernel_size=3, padding=1, key=keys[2])
        self.maxpool2 = nn.MaxPool2d(3, stride=2, use_ceil=True)

        self.inception3a = inception_block(192, 64, 96, 128, 16, 32, 32, key=keys[3])
        self.inception3b = inception_block(256, 128, 128, 192, 32, 96, 64, key=keys[4])
        self.maxpool3 = nn.MaxPool2d(3, stride=2, use_ceil=True)

        self.inception4a = inception_block(480, 192, 96, 208, 16, 48, 64, key=keys[5])
        self.inception4b = inception_block(512, 160, 112, 224, 24, 64, 64, key=keys[6])
        self.inception4c = inception_block(512, 128, 128, 256, 24, 64, 64, key=keys[7])
        self.inception4d = inception_block(512, 112, 144, 288, 32, 64, 64, key=keys[8])
        self.inception4e = inception_block(528, 256, 160, 320, 32, 128, 128, key=keys[9])
        self.maxpool4 = nn.MaxPool2d(2, stride=2, use_ceil=True)

        self.inception5a = inception_block(832, 256, 160, 320, 32, 128, 128, key=keys[10])
        self.inception5b = inception_block(832, 384, 192, 384, 48, 128, 128, key=keys[11])

        self.aux1 = None
        self.aux2 = None
        if aux_logits:
            self.aux1 = inception_aux_block(512, num_classes, dropout=dropout_aux, key=keys[12])
            self.aux2 = inception_aux_block(528, num_classes, dropout=dropout_aux, key=keys[13])

        self.avgpool = nn.AdaptiveAvgPool2d((1, 1))
        self.dropout = nn.Dropout(p=dropout)
        self.fc = nn.Linear(1024, num_classes, key=keys[14])

    @boundary
    def __call__(self, x, *, key=None):                                # reference :117-179
        if key is None:
            raise RuntimeError("The model requires a PRNGKey.")
        _refuse_grad()
        live = nn.dropout_live(self.dropout) or (self.aux_logits and any(nn.dropout_live(getattr(a, "dropout", None))
                                                                         for a in (self.aux1, self.aux2)))
        # jrandom.split(key, 14); keys[14] and keys[15] are clamped to keys[13] by jax.  Only the Dropouts draw from them.
        keys = jr.split(ops._batched_keys(key, x.t.shape[0]), 14) if live else [None] * 14
        x = self.conv1(x)
        x = self.maxpool1(x)
        x = self.conv2(x)
        x = self.conv3(x)
        x = self.maxpool2(x)
        x = self.inception3a(x)
        x = self.inception3b(x)
        x = self.maxpool3(x)
        x = self.inception4a(x)
        if self.aux_logits:
            aux1 = self.aux1(x, key=keys[7])
        x = self.inception4b(x)
        x = self.inception4c(x)
        x = self.inception4d(x)
        if self.aux_logits:
            aux2 = self.aux2(x, key=keys[11])
        x = self.inception4e(x)
        x = self.maxpool4(x)
        x = self.inception5a(x)
        x = self.inception5b(x)
        if type(self.avgpool) is nn.AdaptiveAvgPool2d and head_fp32():
            x = ops.adaptive_avgpool2d(x, self.avgpool.target_shape, out_fp32=True)
        else:
            x = self.avgpool(x)
        x = ops.flatten(x)
        if nn.dropout_live(self.dropout):
            x = self.dropout(x, key=keys[13])
        x = ops.linear_head(x, self.fc)
        if self.aux_logits:
            return x, aux2, aux1
        return x


def googlenet(torch_weights: str = None, **kwargs: Any) -> GoogLeNet:
    """GoogLeNet (Inception v1) from `Going Deeper with Convolutions` (http://arxiv.org/abs/1409.4842).  The minimum input size
    is 15 x 15.  A checkpoint always holds the auxiliary heads: the model is built with them, loaded, and `aux_logits` is switched
    off again unless the caller asked for them."""
    if torch_weights:
        use_aux = kwargs.get("aux_logits", False)
        kwargs = {k: v for k, v in kwargs.items() if k != "aux_logits"}
        model = GoogLeNet(aux_logits=True, **kwargs)
        model = load_torch_weights(model, torch_weights=torch_weights)
        if not use_aux:
            model = _rebuild(model, None, lambda k, v: False if k == "aux_logits" else v)    # (the modules are shared)
        else:
            warnings.warn("Loaded torch_weights weights for GoogLeNet. But, aux-branch weights are un-trained.")
    else:
        model = GoogLeNet(**kwargs)
    return model
