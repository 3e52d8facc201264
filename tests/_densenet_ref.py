"""DenseNet restated with torch.nn.functional in fp64, independently of the package (reference models/classification/densenet.py:
literal concatenation in front of every layer, BatchNorm eps 1e-5, training-mode BatchNorm as a loaded eqx.experimental.BatchNorm),
plus torchvision-named synthetic checkpoints whose classifier weight carries a head scale computed here, on the CPU."""
from __future__ import annotations

from collections import OrderedDict

import numpy as np

from oracle.state import _bn, _conv, _linear, synthetic_images

F32 = np.float32
EPS = 1e-5

# variant -> (growth rate, block config, stem width); bn_size is 4 everywhere (reference :253-302)
VARIANTS = OrderedDict([
    ("densenet121", (32, (6, 12, 24, 16), 64)), ("densenet161", (48, (6, 12, 36, 24), 96)),
    ("densenet169", (32, (6, 12, 32, 32), 64)), ("densenet201", (32, (6, 12, 48, 32), 64)),
])
BN_SIZE = 4
# (input size, batch) of the whole-network tests: the head scale of a variant is chosen for exactly these
CASES = {"densenet121": ((224, 2), (64, 3), (80, 3)), "densenet161": ((64, 2),), "densenet169": ((64, 2),), "densenet201": ((64, 2),)}


def layer_shapes(variant, size=224):
    """[(block, C_in of the layer, map)], [(transition, C_in, map)] for a size x size input: maps 56 / 28 / 14 / 7 at 224."""
    g, cfg, c = VARIANTS[variant]
    h = ((size + 6 - 7) // 2 + 1 + 2 - 3) // 2 + 1
    layers, trans = [], []
    for b, n in enumerate(cfg):
        layers += [(b, c + i * g, h) for i in range(n)]
        c += n * g
        if b != len(cfg) - 1:
            trans.append((b, c, h))
            c, h = c // 2, h // 2
    return layers, trans, c


def _state(variant, seed, num_classes, head_scale):
    g, cfg, c = VARIANTS[variant]
    rng = np.random.Generator(np.random.PCG64(seed))
    sd = OrderedDict()
    _conv(sd, rng, "features.conv0", 3, c, 7, False)
    _bn(sd, rng, "features.norm0", c)
    for b, n in enumerate(cfg, 1):
        for i in range(1, n + 1):
            p = f"features.denseblock{b}.denselayer{i}"
            _bn(sd, rng, p + ".norm1", c)
            _conv(sd, rng, p + ".conv1", c, BN_SIZE * g, 1, False)
            _bn(sd, rng, p + ".norm2", BN_SIZE * g)
            _conv(sd, rng, p + ".conv2", BN_SIZE * g, g, 3, False)
            c += g
        if b != len(cfg):
            _bn(sd, rng, f"features.transition{b}.norm", c)
            _conv(sd, rng, f"features.transition{b}.conv", c, c // 2, 1, False)
            c //= 2
    _bn(sd, rng, "features.norm5", c)
    _linear(sd, rng, "classifier", c, num_classes)
    sd["classifier.weight"] = (sd["classifier.weight"] * F32(head_scale)).astype(F32)
    return sd


def features_torch(sd, variant, x, train=False, new_running=None):
    """fp64 pooled features [B, C] of images x [B, 3, H, W].  train: every BatchNorm is the TRAINING branch of a loaded
    eqx.experimental.BatchNorm: running' = 0.01 batch + 0.99 running (biased batch variance over batch and map) and the layer
    normalises with running'; `new_running[name]` receives (mean', var')."""
    import torch
    import torch.nn.functional as Fn
    g, cfg, _ = VARIANTS[variant]
    t = {k: torch.from_numpy(np.asarray(v, np.float64)) for k, v in sd.items() if np.asarray(v).dtype == F32}

    def bn_relu(v, p):
        rm, rv = t[p + ".running_mean"], t[p + ".running_var"]
        if train:
            m = v.mean((0, 2, 3))
            var = ((v - m.reshape(1, -1, 1, 1)) ** 2).mean((0, 2, 3))
            rm, rv = 0.01 * m + 0.99 * rm, 0.01 * var + 0.99 * rv
            if new_running is not None:
                new_running[p] = (rm.numpy(), rv.numpy())
        return torch.relu(Fn.batch_norm(v, rm, rv, t[p + ".weight"], t[p + ".bias"], False, 0.0, EPS))

    with torch.no_grad():
        v = torch.from_numpy(np.asarray(x, np.float64))
        v = Fn.max_pool2d(bn_relu(Fn.conv2d(v, t["features.conv0.weight"], stride=2, padding=3), "features.norm0"), 3, 2, 1)
        for b, n in enumerate(cfg, 1):
            feats = [v]
            for i in range(1, n + 1):
                p = f"features.denseblock{b}.denselayer{i}"
                cat = torch.cat(feats, 1)                              # the literal concatenation in front of every layer
                mid = Fn.conv2d(bn_relu(cat, p + ".norm1"), t[p + ".conv1.weight"])
                feats.append(Fn.conv2d(bn_relu(mid, p + ".norm2"), t[p + ".conv2.weight"], padding=1))
            v = torch.cat(feats, 1)
            if b != len(cfg):
                p = f"features.transition{b}"
                v = Fn.avg_pool2d(Fn.conv2d(bn_relu(v, p + ".norm"), t[p + ".conv.weight"]), 2, 2)
        return bn_relu(v, "features.norm5").mean((2, 3)).numpy()


def logits(sd, feats):
    return feats @ np.asarray(sd["classifier.weight"], np.float64).T + np.asarray(sd["classifier.bias"], np.float64)


_FEATS = {}


def case_features(variant, seed, size, B):
    """The pooled fp64 features of synthetic_images(B, size, seed) -- independent of the head scale, computed once per process."""
    key = (variant, seed, size, B)
    if key not in _FEATS:
        _FEATS[key] = features_torch(_state(variant, seed, 1000, 1.0), variant, synthetic_images(B, size, seed=seed))
    return _FEATS[key]


def head_scale(variant, seed=1):
    """The pooled features reaching the U(+-1/sqrt(C)) classifier are small.  The classifier WEIGHT is multiplied by this so that the
    largest |logit - bias| over the variant's CASES is around 2: 2 / sqrt(lo * hi) with lo / hi the smallest / largest per-case maximum
    at unit scale, so all cases stay inside [1, 3] as long as hi / lo < 2.25 (the whole-network tests assert the range)."""
    w = np.asarray(_state(variant, seed, 1000, 1.0)["classifier.weight"], np.float64)
    tops = [float(np.abs(case_features(variant, seed, size, B) @ w.T).max()) for size, B in CASES[variant]]
    return 2.0 / float(np.sqrt(min(tops) * max(tops)))


def densenet_state(variant="densenet121", seed=1, num_classes=1000, head_scale_=None):
    """torchvision's registration order: features.conv0, norm0, denseblock{b}.denselayer{l}.(norm1, conv1, norm2, conv2),
    transition{b}.(norm, conv), norm5, classifier.  head_scale_ = None computes `head_scale` (fp64 forwards on the CPU); the host tests
    that never look at logits pass 1.0."""
    s = head_scale(variant, seed) if head_scale_ is None else head_scale_
    return _state(variant, seed, num_classes, s)


def forward_torch(sd, variant, x, train=False, new_running=None):
    return logits(sd, features_torch(sd, variant, x, train=train, new_running=new_running))


def dropout_keys(key, n_features, block_index, n_layers, layer):
    """The key the Dropout of layer `layer` of the block at position `block_index` of `features` is handed, for one sample's key:
    nn.Sequential splits over its layers, the block over its layers, the Dropout uses its share as given (reference :99-101, :66)."""
    from oracle import np_ops as O
    return O.jax_split(O.jax_split(np.asarray(key, np.uint32), n_features)[block_index], n_layers)[layer]
