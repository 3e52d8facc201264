"""SqueezeNet 1.0 / 1.1 restated with torch.nn.functional in fp64, independently of the package (reference
models/classification/squeezenet.py:14-139; max pooling with ceil_mode=True), plus torchvision-named synthetic checkpoints."""
from __future__ import annotations

from collections import OrderedDict

import numpy as np

from oracle.state import _conv

F32 = np.float32

# features index -> "pool" or Fire (inplanes, squeeze, expand1x1, expand3x3); index 0 is the entry convolution (kernel, width)
PLANS = {
    "1_0": ((7, 96), {3: (96, 16, 64, 64), 4: (128, 16, 64, 64), 5: (128, 32, 128, 128), 6: "pool", 7: (256, 32, 128, 128),
                      8: (256, 48, 192, 192), 9: (384, 48, 192, 192), 10: (384, 64, 256, 256), 11: "pool", 12: (512, 64, 256, 256)}),
    "1_1": ((3, 64), {3: (64, 16, 64, 64), 4: (128, 16, 64, 64), 5: "pool", 6: (128, 32, 128, 128), 7: (256, 32, 128, 128), 8: "pool",
                      9: (256, 48, 192, 192), 10: (384, 48, 192, 192), 11: (384, 64, 256, 256), 12: (512, 64, 256, 256)}),
}
FACTORY = {"1_0": "squeezenet1_0", "1_1": "squeezenet1_1"}

# The features reaching the U(+-1/sqrt(512)) final convolution are small (its pooled ReLU outputs are ~0.05 + the bias), so the head
# WEIGHT is multiplied by this: on the CPU, for seed 1 and synthetic_images(2, size, seed=1), the fp64 forward below gives max logit
# 1.27 .. 1.43 and 55 .. 57 % of the logits > 0 for squeezenet1_1 at 64 / 224 px and squeezenet1_0 at 96 / 224 px (16 -> 1.02 .. 1.15,
# 24 -> 1.52 .. 1.73).
HEAD_SCALE = 20.0


def fires(version):
    """[(features index, inplanes, squeeze, expand1x1, expand3x3)] in forward order."""
    return [(i,) + spec for i, spec in sorted(PLANS[version][1].items()) if spec != "pool"]


def squeezenet_state(version, seed=1, num_classes=1000, head_scale=HEAD_SCALE):
    """torchvision's registration order: features.0, then per Fire squeeze / expand1x1 / expand3x3 (weight, bias), then classifier.1."""
    rng = np.random.Generator(np.random.PCG64(seed))
    sd = OrderedDict()
    k, width = PLANS[version][0]
    _conv(sd, rng, "features.0", 3, width, k, True)
    for i, inp, s, e1, e3 in fires(version):
        _conv(sd, rng, f"features.{i}.squeeze", inp, s, 1, True)
        _conv(sd, rng, f"features.{i}.expand1x1", s, e1, 1, True)
        _conv(sd, rng, f"features.{i}.expand3x3", s, e3, 3, True)
    _conv(sd, rng, "classifier.1", 512, num_classes, 1, True)
    sd["classifier.1.weight"] = (sd["classifier.1.weight"] * F32(head_scale)).astype(F32)
    return sd


def forward_torch(sd, version, x, masks=None, device="cpu"):
    """fp64 logits [B, classes] of images x [B, 3, H, W].  `masks`: None (inference) or a bool array [B, 512, h, w], the Dropout keep
    mask of the classifier (p = 0.5: kept values are doubled)."""
    import torch
    import torch.nn.functional as Fn
    t = lambda k: torch.from_numpy(np.asarray(sd[k], np.float64)).to(device)
    conv = lambda y, p, **kw: torch.relu(Fn.conv2d(y, t(p + ".weight"), t(p + ".bias"), **kw))
    y = conv(torch.from_numpy(np.asarray(x, np.float64)).to(device), "features.0", stride=2)
    y = Fn.max_pool2d(y, 3, 2, ceil_mode=True)
    for i, spec in sorted(PLANS[version][1].items()):
        if spec == "pool":
            y = Fn.max_pool2d(y, 3, 2, ceil_mode=True)
            continue
        s = conv(y, f"features.{i}.squeeze")
        y = torch.cat([conv(s, f"features.{i}.expand1x1"), conv(s, f"features.{i}.expand3x3", padding=1)], dim=1)
    if masks is not None:
        y = torch.where(torch.from_numpy(np.asarray(masks, bool)).to(device), y / 0.5, torch.zeros_like(y))
    y = conv(y, "classifier.1")
    return y.mean(dim=(2, 3)).cpu().numpy()


def feature_shape(version, size):
    """(512, h, w) of the map the classifier sees for a size x size input."""
    k = PLANS[version][0][0]
    h = (size - k) // 2 + 1
    n_pool = 1 + sum(1 for v in PLANS[version][1].values() if v == "pool")
    for _ in range(n_pool):
        h = -(-(h - 3) // 2) + 1
    return (512, h, h)


def dropout_masks(version, size, keys, p=0.5):
    """The keep masks eqx.nn.Dropout draws inside `classifier(x, key=key)`: nn.Sequential splits the sample's key in len(layers) = 4,
    Dropout is layer 0; bernoulli(key, 1 - p, (512, h, w)) from the Threefry restatement in oracle.np_ops."""
    from oracle import np_ops as O
    shape = feature_shape(version, size)
    return np.stack([O.jax_bernoulli(O.jax_split(np.asarray(k, np.uint32), 4)[0], 1.0 - p, shape) for k in keys])
