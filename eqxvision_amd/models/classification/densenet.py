"""DenseNet 121 / 161 / 169 / 201 (reference models/classification/densenet.py:15-305).

Same fields / constructors / defaults / parameter order, so `torch_weights=` loads a torchvision-ordered checkpoint.  Device lowering
of the bf16 inference forward:
  * the stem (conv 7x7 + BatchNorm + ReLU + max pool) is ResNet's entry launch (ops.stem_conv_pool);
  * a dense block is ONE [B, H, W, C0 + L * growth] buffer and two launches per layer (ops.dense_block): mv_preact_conv1x1_fwd applies
    BatchNorm 1 + ReLU to the buffer's first C_i channels on their way into LDS, runs the 1x1 and BatchNorm 2 + ReLU into a scratch map;
    mv_conv3x3_slice_fwd writes the 3x3 of that map into channels [C_i, C_i + growth) -- nothing is concatenated;
  * a transition is one launch (ops.dense_transition): BatchNorm + ReLU, the 2 x 2 average IN FRONT of the 1x1 (exact: both are
    linear; a quarter of the product), written straight into the first channels of the NEXT block's buffer; after the stem one
    mv_copy_rows places the block's input;
  * the tail: norm5 + ReLU, the global average in fp32, the flatten, the fp32 classifier;
  * training mode (BatchNorm on batch statistics, live Dropout), fp32 mode, the switches ("no_dense_fused", "force_generic") or foreign
    structures: the literal composition (ops.dense_block_literal / ops.dense_transition_literal).
The key indexing of `__init__` is the reference's, with jax's clamping of out-of-range indices: `keys` is RE-BOUND to a 3-way split
inside the block loop, so from the second block on keys[i * 2 + 1] and every keys[i * 2 + 2] are that split's last element, and the
classifier takes the last element of the last split.  The Dropout schedule: `features` splits the key over its layers, a block
splits its share over its layers, a layer's Dropout draws from its share as given.  No backward: the family refuses inside
filter_value_and_grad.
"""
from __future__ import annotations

from typing import Any, Optional, Sequence, Tuple

from ... import nn, ops
from ... import random as jr
from ..._act import head_fp32
from ..._module import Module
from ...nn import boundary
from ...utils import load_torch_weights


def _refuse_grad():
    from ... import grad as _grad
    if _grad.active():
        # the dense-layer kernels, the concatenation and the average pool have no backward: refuse rather than return a gradient
        # without them
        raise NotImplementedError("DenseNet was launched inside filter_value_and_grad by an op without a backward "
                                  "(eqxvision_amd/grad.py lists what is differentiable)")


def _at(keys, i: int):
    """keys[i] as jax indexes: an out-of-range index is clamped to the last element."""
    return keys[min(i, len(keys) - 1)]


class _DenseLayer(Module):
    norm1: nn.BatchNorm
    relu: nn.Lambda
    conv1: nn.Conv2d
    norm2: nn.BatchNorm
    conv2: nn.Conv2d
    dropout: nn.Dropout

    def __init__(self, num_input_features: int, growth_rate: int, bn_size: int, drop_rate: float, key=None) -> None:
        keys = jr.split(key if key is not None else jr.PRNGKey(0), 2)
        self.norm1 = nn.BatchNorm(num_input_features, axis_name="batch")
        self.relu = nn.Lambda(nn.relu)
        self.conv1 = nn.Conv2d(num_input_features, bn_size * growth_rate, kernel_size=1, stride=1, use_bias=False, key=keys[0])
        self.norm2 = nn.BatchNorm(bn_size * growth_rate, axis_name="batch")
        self.conv2 = nn.Conv2d(bn_size * growth_rate, growth_rate, kernel_size=3, stride=1, padding=1, use_bias=False, key=keys[1])
        self.dropout = nn.Dropout(p=float(drop_rate))

    def __call__(self, x, *, key=None):                                # reference :55-67: one feature map or the list of them
        _refuse_grad()
        feats = list(x) if isinstance(x, (list, tuple)) else [x]
        if not all(ops.is_act(f) for f in feats):
            from ..._act import wrap
            return nn._unwrap(ops.dense_layer_literal([wrap(f, False) for f in feats], self, key), False)
        return ops.dense_layer_literal(feats, self, key)


class _DenseBlock(Module):
    layers: Sequence[Module]
    num_layers: int

    def __init__(self, num_layers: int, num_input_features: int, bn_size: int, growth_rate: int, drop_rate: float, key=None) -> None:
        self.layers = []
        self.num_layers = num_layers
        keys = jr.split(key if key is not None else jr.PRNGKey(0), num_layers)
        for i in range(num_layers):
            self.layers.append(_DenseLayer(num_input_features + i * growth_rate, growth_rate=growth_rate, bn_size=bn_size,
                                           drop_rate=drop_rate, key=keys[i]))

    @boundary
    def __call__(self, x, *, key=None):                                # reference :97-103
        _refuse_grad()
        return ops.dense_block(x, self, key=key)


class _Transition(Module):
    layers: nn.Sequential

    def __init__(self, num_input_features: int, num_output_features: int, key=None) -> None:
        self.layers = nn.Sequential([
            nn.BatchNorm(num_input_features, axis_name="batch"),
            nn.Lambda(nn.relu),
            nn.Conv2d(num_input_features, num_output_features, kernel_size=1, stride=1, use_bias=False, key=key),
            nn.AvgPool2d(kernel_size=2, stride=2),
        ])

    @boundary
    def __call__(self, x, *, key=None):                                # reference :132-133
        _refuse_grad()
        return ops.dense_transition(x, self, key=key)


class DenseNet(Module):
    """A simple port of `torchvision.models.densenet`."""

    features: nn.Sequential
    classifier: nn.Linear

    def __init__(self, growth_rate: int = 32, block_config: Tuple[int, int, int, int] = (6, 12, 24, 16), num_init_features: int = 64,
                 bn_size: int = 4, drop_rate: float = 0, num_classes: int = 1000, *, key=None) -> None:
        if key is None:
            key = jr.PRNGKey(0)
        keys = jr.split(key, 2 * len(block_config) + 2)
        features = [
            nn.Conv2d(3, num_init_features, kernel_size=7, stride=2, padding=3, use_bias=False, key=keys[0]),
            nn.BatchNorm(num_init_features, axis_name="batch"),
            nn.Lambda(nn.relu),
            nn.MaxPool2d(kernel_size=3, stride=2, padding=1),
        ]
        num_features = num_init_features
        for i, num_layers in enumerate(block_config):
            keys = jr.split(_at(keys, i * 2 + 1), 3)                   # the reference re-binds `keys` here (:188)
            features.append(_DenseBlock(num_layers=num_layers, num_input_features=num_features, bn_size=bn_size,
                                        growth_rate=growth_rate, drop_rate=drop_rate, key=keys[0]))
            num_features = num_features + num_layers * growth_rate
            if i != len(block_config) - 1:
                features.append(_Transition(num_input_features=num_features, num_output_features=num_features // 2,
                                            key=_at(keys, i * 2 + 2)))
                num_features = num_features // 2
        features.extend([nn.BatchNorm(num_features, axis_name="batch"), nn.Lambda(nn.relu), nn.AdaptiveAvgPool2d((1, 1))])
        self.features = nn.Sequential(features)
        self.classifier = nn.Linear(num_features, num_classes, key=keys[-1])

    def _reference_layout(self) -> bool:
        """The feature list the constructor builds: the stem, blocks and transitions alternating, norm5 + ReLU + the global average."""
        L = self.features.layers
        if len(L) < 8 or not (type(L[0]) is nn.Conv2d and type(L[1]) is nn.BatchNorm and isinstance(L[2], nn.Lambda)
                              and nn.act_name(L[2].fn) == "relu" and type(L[3]) is nn.MaxPool2d and not L[3].use_ceil):
            return False
        if not (type(L[-3]) is nn.BatchNorm and isinstance(L[-2], nn.Lambda) and nn.act_name(L[-2].fn) == "relu"
                and type(L[-1]) is nn.AdaptiveAvgPool2d and L[-1].target_shape == (1, 1)):
            return False
        body = L[4:-3]
        return (len(body) % 2 == 1 and all(isinstance(m, _DenseBlock) for m in body[0::2])
                and all(isinstance(m, _Transition) for m in body[1::2]) and isinstance(self.classifier, nn.Linear))

    @boundary
    def __call__(self, x, *, key=None):                                # reference :220-229
        if key is None:
            raise RuntimeError("The model requires a PRNGKey.")
        _refuse_grad()
        if not self._reference_layout():
            return self.classifier(ops.flatten(self.features(x, key=key)))
        L = self.features.layers
        body = L[4:-3]
        live = any(nn.dropout_live(getattr(l, "dropout", None)) for b in body[0::2] for l in b.layers)
        # nn.Sequential splits its key over its layers; only the blocks' Dropouts draw from their share
        keys = jr.split(ops._batched_keys(key, x.t.shape[0]), len(L)) if live else [None] * len(L)
        x = ops.stem_conv_pool(x, L[0], L[1], "relu", L[3])
        filled = None
        for j, m in enumerate(body):
            if isinstance(m, _DenseBlock):
                x = ops.dense_block(x, m, filled=filled, key=keys[4 + j])
                filled = None
                continue
            # a transition writes into the next block's buffer when that block takes the two-launch path
            B, H, W, C = x.t.shape
            nxt, n_out = body[j + 1], m.layers.layers[2].out_channels
            plan = ops.dense_block_plan(nxt, n_out, H // 2, W // 2) if H >= 2 and W >= 2 else None
            x = ops.dense_transition(x, m, plan[2] if plan else 0)
            filled = n_out if plan and x.t.shape[-1] == plan[2] else None
        x = ops.batchnorm(x, L[-3], "relu")
        x = ops.adaptive_avgpool2d(x, (1, 1), out_fp32=True) if head_fp32() else L[-1](x)
        return ops.linear_head(ops.flatten(x), self.classifier)


def _densenet(growth_rate: int, block_config: Tuple[int, int, int, int], num_init_features: int, **kwargs: Any) -> DenseNet:
    return DenseNet(growth_rate, block_config, num_init_features, **kwargs)


def _variant(name, growth_rate, block_config, num_init_features):
    def make(torch_weights: Optional[str] = None, **kwargs: Any) -> DenseNet:
        model = _densenet(growth_rate, block_config, num_init_features, **kwargs)
        if torch_weights:
            model = load_torch_weights(model, torch_weights=torch_weights)
        return model

    make.__name__ = make.__qualname__ = name
    make.__doc__ = (f"{name} from `Densely Connected Convolutional Networks` (https://arxiv.org/pdf/1608.06993.pdf).  The minimum "
                    "input size is 29 x 29.  `torch_weights`: torchvision checkpoint path / URL.")
    return make


densenet121 = _variant("densenet121", 32, (6, 12, 24, 16), 64)
densenet161 = _variant("densenet161", 48, (6, 12, 36, 24), 96)
densenet169 = _variant("densenet169", 32, (6, 12, 32, 32), 64)
densenet201 = _variant("densenet201", 32, (6, 12, 48, 32), 64)
