"""GoogLeNet restated with torch.nn.functional in fp64, independently of the package (reference models/classification/googlenet.py:
BatchNorm eps 1e-3, equinox's ceil-mode pooling size rule, equinox's adaptive-pool bounds, CHW ravel in the auxiliary heads, the 3x3
"5x5" branch), plus a torchvision-named synthetic checkpoint and the Dropout keep masks of the reference's key schedule."""
from __future__ import annotations

from collections import OrderedDict

import numpy as np

from oracle.state import _bn, _conv, _linear

F32 = np.float32
EPS = 1e-3

# name -> (in, ch1x1, ch3x3red, ch3x3, ch5x5red, ch5x5, pool_proj), in forward order (reference :83-100)
INCEPTIONS = OrderedDict([
    ("inception3a", (192, 64, 96, 128, 16, 32, 32)), ("inception3b", (256, 128, 128, 192, 32, 96, 64)),
    ("inception4a", (480, 192, 96, 208, 16, 48, 64)), ("inception4b", (512, 160, 112, 224, 24, 64, 64)),
    ("inception4c", (512, 128, 128, 256, 24, 64, 64)), ("inception4d", (512, 112, 144, 288, 32, 64, 64)),
    ("inception4e", (528, 256, 160, 320, 32, 128, 128)), ("inception5a", (832, 256, 160, 320, 32, 128, 128)),
    ("inception5b", (832, 384, 192, 384, 48, 128, 128)),
])
MAP_224 = {"inception3a": 28, "inception3b": 28, "inception4a": 14, "inception4b": 14, "inception4c": 14, "inception4d": 14,
           "inception4e": 14, "inception5a": 7, "inception5b": 7}

# The pooled 1024 features reaching the U(+-1/32) classifier are small: the head WEIGHTS (fc, aux*.fc2) are multiplied by these so
# that max |logit| is around 2.  On the CPU with the fp64 forward below, seed 1, synthetic_images(2, 224, seed=1) and (3, 75, seed=1),
# unit scales give max |logit - bias| = 0.20 / 0.19 (fc), 0.094 / 0.094 (aux2.fc2) and 0.109 / 0.111 (aux1.fc2), half of the logits > 0.
HEAD_SCALE = 9.0
AUX_SCALE = 18.0
# Training mode: Dropout(0.7) multiplies the kept fc1 features of an auxiliary head by 1 / 0.3, and the fp64 forward below (seed 1,
# synthetic_images(4, 75, seed=1), the masks of PRNGKey(7)) gives max |aux logit| 3.19 / 3.49 at AUX_SCALE -- not the "around 2" the
# absolute logit tolerances of the project are meant for.  A training-mode checkpoint is written with this scale instead: 1.8 / 1.95.
AUX_SCALE_TRAIN = 10.0


def _basic(sd, rng, name, cin, cout, k):
    _conv(sd, rng, name + ".conv", cin, cout, k, False)
    _bn(sd, rng, name + ".bn", cout)


def googlenet_state(seed=1, num_classes=1000, head_scale=HEAD_SCALE, aux_scale=AUX_SCALE):
    """torchvision's registration order: conv1 .. conv3, the nine modules (branch1, branch2.0, branch2.1, branch3.0, branch3.1,
    branch4.1), aux1, aux2 (conv, fc1, fc2), fc."""
    rng = np.random.Generator(np.random.PCG64(seed))
    sd = OrderedDict()
    _basic(sd, rng, "conv1", 3, 64, 7)
    _basic(sd, rng, "conv2", 64, 64, 1)
    _basic(sd, rng, "conv3", 64, 192, 3)
    for name, (cin, c1, c3r, c3, c5r, c5, cp) in INCEPTIONS.items():
        _basic(sd, rng, name + ".branch1", cin, c1, 1)
        _basic(sd, rng, name + ".branch2.0", cin, c3r, 1)
        _basic(sd, rng, name + ".branch2.1", c3r, c3, 3)
        _basic(sd, rng, name + ".branch3.0", cin, c5r, 1)
        _basic(sd, rng, name + ".branch3.1", c5r, c5, 3)
        _basic(sd, rng, name + ".branch4.1", cin, cp, 1)
    for name, cin in (("aux1", 512), ("aux2", 528)):
        _basic(sd, rng, name + ".conv", cin, 128, 1)
        _linear(sd, rng, name + ".fc1", 2048, 1024)
        _linear(sd, rng, name + ".fc2", 1024, num_classes)
        sd[name + ".fc2.weight"] = (sd[name + ".fc2.weight"] * F32(aux_scale)).astype(F32)
    _linear(sd, rng, "fc", 1024, num_classes)
    sd["fc.weight"] = (sd["fc.weight"] * F32(head_scale)).astype(F32)
    return sd


def ceil_pool_size(n, k, s):
    """equinox's use_ceil rule without padding: a remainder grows the output by one."""
    return (n - k) // s + 1 + (1 if (n - k) % s else 0)


def adaptive_bounds(n, t):
    """equinox's AdaptiveAvgPool: equal chunks when divisible, else the first n % t outputs take n // t + 1 inputs, the rest n // t."""
    k, big = n // t, n % t
    out, pos = [], 0
    for i in range(t):
        sz = k + 1 if i < big else k
        out.append((pos, pos + sz))
        pos += sz
    return out


def map_sizes(size):
    """(the map the modules of stage 3 see, stage 4, stage 5) for a size x size input."""
    h = (size + 6 - 7) // 2 + 1
    h = ceil_pool_size(h, 3, 2)
    h3 = ceil_pool_size(h, 3, 2)
    h4 = ceil_pool_size(h3, 3, 2)
    return h3, h4, ceil_pool_size(h4, 2, 2)


def forward_torch(sd, x, aux=True, train=False, masks=None, device="cpu", new_running=None):
    """fp64 outputs (logits, aux2, aux1) -- or the logits alone with aux=False -- of images x [B, 3, H, W].
    train: every BatchNorm is the TRAINING branch of a loaded eqx.experimental.BatchNorm: running' = 0.01 batch + 0.99 running (biased
    batch variance over batch and map), and the layer normalises with running'; `new_running[name]` receives (mean', var').
    masks: None or a dict {"main": bool [B, 1024], "aux1": bool [B, 1024], "aux2": ...}: the Dropout keep masks (p = 0.2 / 0.7)."""
    import torch
    import torch.nn.functional as Fn
    t = {k: torch.from_numpy(np.asarray(v, np.float64)).to(device) for k, v in sd.items() if np.asarray(v).dtype == F32}

    def basic(v, p, **kw):
        v = Fn.conv2d(v, t[p + ".conv.weight"], **kw)
        rm, rv = t[p + ".bn.running_mean"], t[p + ".bn.running_var"]
        if train:
            m = v.mean((0, 2, 3))
            var = ((v - m.reshape(1, -1, 1, 1)) ** 2).mean((0, 2, 3))
            rm, rv = 0.01 * m + 0.99 * rm, 0.01 * var + 0.99 * rv
            if new_running is not None:
                new_running[p + ".bn"] = (rm.cpu().numpy(), rv.cpu().numpy())
        return torch.relu(Fn.batch_norm(v, rm, rv, t[p + ".bn.weight"], t[p + ".bn.bias"], False, 0.0, EPS))

    def ceil_pool(v, k, s):
        out = Fn.max_pool2d(v, k, s, ceil_mode=True)
        assert tuple(out.shape[2:]) == (ceil_pool_size(v.shape[2], k, s), ceil_pool_size(v.shape[3], k, s))
        return out

    def inception(v, p):
        b1 = basic(v, p + ".branch1")
        b2 = basic(basic(v, p + ".branch2.0"), p + ".branch2.1", padding=1)
        b3 = basic(basic(v, p + ".branch3.0"), p + ".branch3.1", padding=1)
        b4 = basic(Fn.max_pool2d(v, 3, 1, 1), p + ".branch4.1")
        return torch.cat([b1, b2, b3, b4], 1)

    def drop(v, name, p):
        if masks is None or name not in masks:
            return v
        keep = torch.from_numpy(np.asarray(masks[name], bool)).to(device)
        return torch.where(keep, v / (1.0 - p), torch.zeros_like(v))

    def aux_head(v, p):
        hb, wb = adaptive_bounds(v.shape[2], 4), adaptive_bounds(v.shape[3], 4)
        v = torch.stack([torch.stack([v[:, :, h0:h1, w0:w1].mean((2, 3)) for (w0, w1) in wb], -1) for (h0, h1) in hb], -2)   # [B,C,4,4]
        v = basic(v, p + ".conv")
        v = v.reshape(v.shape[0], -1)                                  # NCHW: the ravel of the (C, H, W) sample
        v = torch.relu(v @ t[p + ".fc1.weight"].T + t[p + ".fc1.bias"])
        v = drop(v, p, 0.7)
        return v @ t[p + ".fc2.weight"].T + t[p + ".fc2.bias"]

    with torch.no_grad():
        v = torch.from_numpy(np.asarray(x, np.float64)).to(device)
        v = ceil_pool(basic(v, "conv1", stride=2, padding=3), 3, 2)
        v = ceil_pool(basic(basic(v, "conv2"), "conv3", padding=1), 3, 2)
        v = ceil_pool(inception(inception(v, "inception3a"), "inception3b"), 3, 2)
        v = inception(v, "inception4a")
        a1 = aux_head(v, "aux1") if aux else None
        v = inception(inception(inception(v, "inception4b"), "inception4c"), "inception4d")
        a2 = aux_head(v, "aux2") if aux else None
        v = ceil_pool(inception(v, "inception4e"), 2, 2)
        v = inception(inception(v, "inception5a"), "inception5b")
        v = drop(v.mean((2, 3)), "main", 0.2)
        y = v @ t["fc.weight"].T + t["fc.bias"]
    if aux:
        return y.cpu().numpy(), a2.cpu().numpy(), a1.cpu().numpy()
    return y.cpu().numpy()


def dropout_masks(keys, aux=True):
    """The keep masks of the reference's key schedule for per-sample keys [B, 2]: the forward splits the key in 14; the main Dropout
    (p = 0.2) is handed keys[15], which jax clamps to keys[13]; aux1 / aux2 get keys[7] / keys[11], split them in 2 and hand their
    Dropout (p = 0.7) the second; bernoulli(key, 1 - p, (1024,)) from the Threefry restatement in oracle.np_ops."""
    from oracle import np_ops as O
    out = {"main": [], "aux1": [], "aux2": []}
    for k in keys:
        ks = O.jax_split(np.asarray(k, np.uint32), 14)
        out["main"].append(O.jax_bernoulli(ks[13], 1.0 - 0.2, (1024,)))
        out["aux1"].append(O.jax_bernoulli(O.jax_split(ks[7], 2)[1], 1.0 - 0.7, (1024,)))
        out["aux2"].append(O.jax_bernoulli(O.jax_split(ks[11], 2)[1], 1.0 - 0.7, (1024,)))
    out = {k: np.stack(v) for k, v in out.items()}
    if not aux:
        out = {"main": out["main"]}
    return out
