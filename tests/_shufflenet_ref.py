"""ShuffleNetV2 restated twice, independently of the package (reference models/classification/shufflenetv2.py:16-230): once in numpy
(fp64, one sample), once with torch.nn.functional (fp64, batched), plus torchvision-named synthetic checkpoints."""
from __future__ import annotations

from collections import OrderedDict

import numpy as np

from oracle.state import _bn, _conv, _linear

F32 = np.float32
EPS = 1e-5

# (stages_repeats, stages_out_channels)
SETTINGS = {
    "shufflenet_v2_x0_5": ((4, 8, 4), (24, 48, 96, 192, 1024)),
    "shufflenet_v2_x1_0": ((4, 8, 4), (24, 116, 232, 464, 1024)),
    "shufflenet_v2_x1_5": ((4, 8, 4), (24, 176, 352, 704, 1024)),
    "shufflenet_v2_x2_0": ((4, 8, 4), (24, 244, 488, 976, 2048)),
}
SMALL = ((2, 3, 2), (8, 20, 36, 72, 64))        # branch widths 10 / 18 / 36: bf % 8 != 0 and odd bf // 2


def _units(setting):
    """[(prefix, inp, oup, stride)] in forward order."""
    repeats, widths = setting
    out, cin = [], widths[0]
    for si, (n, cout) in enumerate(zip(repeats, widths[1:4])):
        for i in range(n):
            out.append((f"stage{si + 2}.{i}", cin if i == 0 else cout, cout, 2 if i == 0 else 1))
        cin = cout
    return out


def shufflenet_state(setting, seed=1, num_classes=1000, head_scale=6.0):
    """torchvision's registration order: convolutions U(+-1/sqrt(fan)), BatchNorms as oracle.state._bn (gamma ~ U[0.5, 1.5], running
    variance ~ U[0.5, 1.5]).  The pooled conv5 features of a 224 input are small against the U(+-1/32) head, so the head weight is
    multiplied by `head_scale`: 6 puts max |logit| at 1.2 - 1.5 for the four factories (window [0.5, 3], as the ConvNeXt state)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    sd = OrderedDict()
    repeats, widths = setting
    _conv(sd, rng, "conv1.0", 3, widths[0], 3, False)
    _bn(sd, rng, "conv1.1", widths[0])
    for p, inp, oup, stride in _units(setting):
        bf = oup // 2
        if stride == 2:
            _conv(sd, rng, p + ".branch1.0", inp, inp, 3, False, groups=inp)
            _bn(sd, rng, p + ".branch1.1", inp)
            _conv(sd, rng, p + ".branch1.2", inp, bf, 1, False)
            _bn(sd, rng, p + ".branch1.3", bf)
        _conv(sd, rng, p + ".branch2.0", inp if stride == 2 else bf, bf, 1, False)
        _bn(sd, rng, p + ".branch2.1", bf)
        _conv(sd, rng, p + ".branch2.3", bf, bf, 3, False, groups=bf)
        _bn(sd, rng, p + ".branch2.4", bf)
        _conv(sd, rng, p + ".branch2.5", bf, bf, 1, False)
        _bn(sd, rng, p + ".branch2.6", bf)
    _conv(sd, rng, "conv5.0", widths[3], widths[4], 1, False)
    _bn(sd, rng, "conv5.1", widths[4])
    _linear(sd, rng, "fc", widths[4], num_classes)
    sd["fc.weight"] = (sd["fc.weight"] * F32(head_scale)).astype(F32)
    return sd


# ----------------------------------------------------------------------------------------------- numpy (fp64), one sample (C,H,W)
def _np_conv(x, w, stride, pad, groups):
    C, H, W = x.shape
    O_, cg, kh, kw = w.shape
    xp = np.pad(x, ((0, 0), (pad, pad), (pad, pad)))
    Ho, Wo = (H + 2 * pad - kh) // stride + 1, (W + 2 * pad - kw) // stride + 1
    y = np.zeros((O_, Ho, Wo))
    og = O_ // groups
    for r in range(kh):
        for s in range(kw):
            patch = xp[:, r:r + stride * (Ho - 1) + 1:stride, s:s + stride * (Wo - 1) + 1:stride]
            if groups == 1:
                y += np.einsum("oc,chw->ohw", w[:, :, r, s], patch)
            elif cg == 1 and og == 1:
                y += w[:, 0, r, s].reshape(-1, 1, 1) * patch
            else:
                raise NotImplementedError
    return y


def _np_bn(x, sd, p):
    g = lambda k: np.asarray(sd[p + k], np.float64).reshape(-1, 1, 1)
    return (x - g(".running_mean")) / np.sqrt(g(".running_var") + EPS) * g(".weight") + g(".bias")


def _np_maxpool3s2(x):
    C, H, W = x.shape
    xp = np.pad(x, ((0, 0), (1, 1), (1, 1)), constant_values=-np.inf)
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    y = np.full((C, Ho, Wo), -np.inf)
    for r in range(3):
        for s in range(3):
            y = np.maximum(y, xp[:, r:r + 2 * (Ho - 1) + 1:2, s:s + 2 * (Wo - 1) + 1:2])
    return y


def np_stem(sd, img):
    """conv1 + BatchNorm + relu + maxpool of one sample (C,H,W), fp64."""
    x = _np_conv(np.asarray(img, np.float64), np.asarray(sd["conv1.0.weight"], np.float64), 2, 1, 1)
    return _np_maxpool3s2(np.maximum(_np_bn(x, sd, "conv1.1"), 0.0))


def forward_numpy(sd, setting, img, shuffle=True):
    w = lambda k: np.asarray(sd[k + ".weight"], np.float64)
    relu = lambda v: np.maximum(v, 0.0)
    x = np_stem(sd, img)
    for p, inp, oup, stride in _units(setting):
        bf = oup // 2

        def branch2(t):
            t = relu(_np_bn(_np_conv(t, w(p + ".branch2.0"), 1, 0, 1), sd, p + ".branch2.1"))
            t = _np_bn(_np_conv(t, w(p + ".branch2.3"), stride, 1, bf), sd, p + ".branch2.4")
            return relu(_np_bn(_np_conv(t, w(p + ".branch2.5"), 1, 0, 1), sd, p + ".branch2.6"))

        if stride == 1:
            out = np.concatenate([x[:bf], branch2(x[bf:])], 0)
        else:
            t = _np_bn(_np_conv(x, w(p + ".branch1.0"), stride, 1, inp), sd, p + ".branch1.1")
            t = relu(_np_bn(_np_conv(t, w(p + ".branch1.2"), 1, 0, 1), sd, p + ".branch1.3"))
            out = np.concatenate([t, branch2(x)], 0)
        if shuffle:
            C, H, W = out.shape
            out = out.reshape(2, C // 2, H, W).transpose(1, 0, 2, 3).reshape(C, H, W)
        x = out
    x = relu(_np_bn(_np_conv(x, w("conv5.0"), 1, 0, 1), sd, "conv5.1"))
    return x.mean((1, 2)) @ w("fc").T + np.asarray(sd["fc.bias"], np.float64)


# ----------------------------------------------------------------------------------------------- torch.nn.functional (fp64), batched
def forward_torch(sd, setting, x, device="cpu", train_bn=False, shuffle=True):
    """x (B,3,H,W) -> numpy logits, fp64 torch ops on `device`.  train_bn: every BatchNorm as the TRAINING branch of a LOADED
    eqx.experimental.BatchNorm (oracle.np_ops.batchnorm_train, not its first call): running' = (1 - momentum) * batch + momentum *
    running with momentum 0.99 and the biased batch variance, and the layer normalises with running'."""
    import torch
    import torch.nn.functional as F
    t = {k: torch.from_numpy(np.asarray(v, np.float64)).to(device) for k, v in sd.items() if np.asarray(v).dtype == F32}

    def bn(v, p):
        if train_bn:
            m = v.mean((0, 2, 3))
            var = ((v - m.reshape(1, -1, 1, 1)) ** 2).mean((0, 2, 3))
            rm, rv = 0.01 * m + 0.99 * t[p + ".running_mean"], 0.01 * var + 0.99 * t[p + ".running_var"]
            return F.batch_norm(v, rm, rv, t[p + ".weight"], t[p + ".bias"], False, 0.0, EPS)
        return F.batch_norm(v, t[p + ".running_mean"], t[p + ".running_var"], t[p + ".weight"], t[p + ".bias"], False, 0.0, EPS)

    with torch.no_grad():
        v = torch.from_numpy(np.asarray(x, np.float64)).to(device)
        v = F.relu(bn(F.conv2d(v, t["conv1.0.weight"], stride=2, padding=1), "conv1.1"))
        v = F.max_pool2d(v, 3, 2, 1)
        for p, inp, oup, stride in _units(setting):
            bf = oup // 2

            def branch2(u):
                u = F.relu(bn(F.conv2d(u, t[p + ".branch2.0.weight"]), p + ".branch2.1"))
                u = bn(F.conv2d(u, t[p + ".branch2.3.weight"], stride=stride, padding=1, groups=bf), p + ".branch2.4")
                return F.relu(bn(F.conv2d(u, t[p + ".branch2.5.weight"]), p + ".branch2.6"))

            if stride == 1:
                out = torch.cat([v[:, :bf], branch2(v[:, bf:])], 1)
            else:
                u = bn(F.conv2d(v, t[p + ".branch1.0.weight"], stride=stride, padding=1, groups=inp), p + ".branch1.1")
                u = F.relu(bn(F.conv2d(u, t[p + ".branch1.2.weight"]), p + ".branch1.3"))
                out = torch.cat([u, branch2(v)], 1)
            if shuffle:
                B, C, H, W = out.shape
                out = out.reshape(B, 2, C // 2, H, W).transpose(1, 2).reshape(B, C, H, W)
            v = out
        v = F.relu(bn(F.conv2d(v, t["conv5.0.weight"]), "conv5.1"))
        return F.linear(v.mean((2, 3)), t["fc.weight"], t["fc.bias"]).cpu().numpy()
