"""ConvNeXt restated twice, independently of the package (reference models/classification/convnext.py:16-220): once in numpy, once
with torch.nn.functional (fp64, CPU), plus torchvision-named synthetic checkpoints.  Stochastic depth draws its per-channel masks
from the reference's key tree (features -> stage -> block -> split(key, 2)[1]) with the Threefry restatement of oracle.np_ops."""
from __future__ import annotations

from collections import OrderedDict

import numpy as np

from oracle import np_ops as O
from oracle.state import _conv, _linear

F32 = np.float32

SETTINGS = {
    "convnext_tiny": ((96, 192, 3), (192, 384, 3), (384, 768, 9), (768, None, 3)),
    "convnext_small": ((96, 192, 3), (192, 384, 3), (384, 768, 27), (768, None, 3)),
    "convnext_base": ((128, 256, 3), (256, 512, 3), (512, 1024, 27), (1024, None, 3)),
    "convnext_large": ((192, 384, 3), (384, 768, 3), (768, 1536, 27), (1536, None, 3)),
}
DEFAULT_SD = {"convnext_tiny": 0.1, "convnext_small": 0.4, "convnext_base": 0.5, "convnext_large": 0.5}


def _ln_near(sd, rng, name, c):
    sd[name + ".weight"] = (1.0 + 0.1 * rng.standard_normal(c)).astype(F32)
    sd[name + ".bias"] = (0.05 * rng.standard_normal(c)).astype(F32)


def convnext_state(setting, seed=1, num_classes=1000, head_scale=None):
    """torchvision's registration order: a block lists its own `layer_scale` before `block.0/2/3/5`.  layer_scale uniform in
    [0.2, 1] (the blocks matter), LayerNorm affines near 1 / 0, the head scaled so that |logit| is ~1-2."""
    rng = np.random.Generator(np.random.PCG64(seed))
    sd = OrderedDict()
    c0 = setting[0][0]
    _conv(sd, rng, "features.0.0", 3, c0, 4, True)
    _ln_near(sd, rng, "features.0.1", c0)
    fi = 1
    for cin, cout, n in setting:
        for bi in range(n):
            p = f"features.{fi}.{bi}"
            sd[p + ".layer_scale"] = rng.uniform(0.2, 1.0, (cin, 1, 1)).astype(F32)
            _conv(sd, rng, p + ".block.0", cin, cin, 7, True, groups=cin)
            _ln_near(sd, rng, p + ".block.2", cin)
            _linear(sd, rng, p + ".block.3", cin, 4 * cin)
            _linear(sd, rng, p + ".block.5", 4 * cin, cin)
        fi += 1
        if cout is not None:
            _ln_near(sd, rng, f"features.{fi}.0", cin)
            _conv(sd, rng, f"features.{fi}.1", cin, cout, 2, True)
            fi += 1
    last = setting[-1][1] or setting[-1][0]
    _ln_near(sd, rng, "classifier.0", last)
    _linear(sd, rng, "classifier.2", last, num_classes)
    sd["classifier.2.weight"] = (sd["classifier.2.weight"] * F32(head_scale if head_scale is not None else 1.0)).astype(F32)
    return sd


def _blocks(sd, setting):
    """[(kind, prefix, ...)] in forward order."""
    out = [("stem", "features.0")]
    fi = 1
    total = sum(n for _, _, n in setting)
    bid = 0
    for cin, cout, n in setting:
        out.append(("stage", f"features.{fi}", n, bid, total))
        bid += n
        fi += 1
        if cout is not None:
            out.append(("down", f"features.{fi}"))
            fi += 1
    return out


def _sd_probs(p, setting):
    total = sum(n for _, _, n in setting)
    return [p * i / (total - 1.0) for i in range(total)]


def _block_keys(key, setting):
    """Per block, the DropPath key of the reference's key tree for one sample's key."""
    n_layers = 1 + len(setting) + sum(1 for _, c, _ in setting if c is not None)
    lk = O.jax_split(np.asarray(key, np.uint32), n_layers)
    out = []
    li = 1
    for cin, cout, n in setting:
        bk = O.jax_split(lk[li], n)
        out += [O.jax_split(bk[j], 2)[1] for j in range(n)]
        li += 1 + (cout is not None)
    return out


def _masks(keys_b, probs, widths):
    """Per block: the (C,) scale bernoulli(key, 1 - p) / (1 - p) of DropPath(mode="local"), or None at p == 0."""
    out = []
    for k, p, c in zip(keys_b, probs, widths):
        if p == 0.0:
            out.append(None)
            continue
        keep = F32(1.0 - p)
        m = O.jax_bernoulli(k, keep, (c,)).astype(np.float64)
        out.append(m / float(keep) if keep > 0 else m)
    return out


def _widths(setting):
    return [cin for cin, _, n in setting for _ in range(n)]


# ----------------------------------------------------------------------------------------------- numpy (fp64), one sample (C,H,W)
def _np_ln_c(x, w, b, eps):
    m = x.mean(0, keepdims=True)
    v = ((x - m) ** 2).mean(0, keepdims=True)
    return (x - m) / np.sqrt(v + eps) * w.reshape(-1, 1, 1) + b.reshape(-1, 1, 1)


def _np_conv64(x, w, b, stride, pad, groups):
    C, H, W = x.shape
    O_, cg, kh, kw = w.shape
    xp = np.pad(x, ((0, 0), (pad, pad), (pad, pad)))
    Ho, Wo = (H + 2 * pad - kh) // stride + 1, (W + 2 * pad - kw) // stride + 1
    y = np.zeros((O_, Ho, Wo))
    og = O_ // groups
    for g in range(groups):
        xs = xp[g * cg:(g + 1) * cg]
        for r in range(kh):
            for s in range(kw):
                patch = xs[:, r:r + stride * Ho:stride, s:s + stride * Wo:stride]           # (cg, Ho, Wo)
                y[g * og:(g + 1) * og] += np.einsum("oc,chw->ohw", w[g * og:(g + 1) * og, :, r, s].astype(np.float64), patch)
    return y + np.asarray(b, np.float64).reshape(-1, 1, 1)


def _np_gelu(x):
    return 0.5 * x * (1.0 + np.tanh(np.sqrt(2.0 / np.pi) * (x + 0.044715 * x ** 3)))


def forward_numpy(sd, setting, img, masks=None):
    """One sample, fp64 numpy.  masks: per-block (C,) scales (training mode) or None."""
    g = lambda k: np.asarray(sd[k], np.float64)
    x = _np_conv64(np.asarray(img, np.float64), g("features.0.0.weight"), g("features.0.0.bias"), 4, 0, 1)
    x = _np_ln_c(x, g("features.0.1.weight"), g("features.0.1.bias"), 1e-6)
    bi = 0
    for kind, pre, *rest in _blocks(sd, setting)[1:]:
        if kind == "down":
            x = _np_ln_c(x, g(pre + ".0.weight"), g(pre + ".0.bias"), 1e-6)
            x = _np_conv64(x, g(pre + ".1.weight"), g(pre + ".1.bias"), 2, 0, 1)
            continue
        for j in range(rest[0]):
            p = f"{pre}.{j}"
            C = x.shape[0]
            h = _np_conv64(x, g(p + ".block.0.weight"), g(p + ".block.0.bias"), 1, 3, C)
            h = _np_ln_c(h, g(p + ".block.2.weight"), g(p + ".block.2.bias"), 1e-5)
            t = h.reshape(C, -1).T @ g(p + ".block.3.weight").T + g(p + ".block.3.bias")
            t = _np_gelu(t) @ g(p + ".block.5.weight").T + g(p + ".block.5.bias")
            r = t.T.reshape(x.shape) * g(p + ".layer_scale")
            if masks is not None and masks[bi] is not None:
                r = r * masks[bi].reshape(-1, 1, 1)
            x = x + r
            bi += 1
    v = x.mean((1, 2))
    m = v.mean()
    v = (v - m) / np.sqrt(((v - m) ** 2).mean() + 1e-6) * g("classifier.0.weight") + g("classifier.0.bias")
    return v @ g("classifier.2.weight").T + g("classifier.2.bias")


# ----------------------------------------------------------------------------------------------- torch.nn.functional (fp64), batched
def forward_torch(sd, setting, imgs, masks=None, device="cpu"):
    """imgs (B,3,H,W); masks: [sample][block] (C,) scales or None.  fp64 on `device`, numpy logits back."""
    import torch
    import torch.nn.functional as F
    t = {k: torch.from_numpy(np.asarray(v, np.float64)).to(device) for k, v in sd.items() if np.asarray(v).dtype == F32}

    def ln_c(x, w, b, eps):
        return F.layer_norm(x.permute(0, 2, 3, 1), (x.shape[1],), w, b, eps).permute(0, 3, 1, 2)

    with torch.no_grad():
        x = torch.from_numpy(np.asarray(imgs, np.float64)).to(device)
        x = F.conv2d(x, t["features.0.0.weight"], t["features.0.0.bias"], stride=4)
        x = ln_c(x, t["features.0.1.weight"], t["features.0.1.bias"], 1e-6)
        bi = 0
        for kind, pre, *rest in _blocks(sd, setting)[1:]:
            if kind == "down":
                x = ln_c(x, t[pre + ".0.weight"], t[pre + ".0.bias"], 1e-6)
                x = F.conv2d(x, t[pre + ".1.weight"], t[pre + ".1.bias"], stride=2)
                continue
            for j in range(rest[0]):
                p = f"{pre}.{j}"
                C = x.shape[1]
                h = F.conv2d(x, t[p + ".block.0.weight"], t[p + ".block.0.bias"], padding=3, groups=C).permute(0, 2, 3, 1)
                h = F.layer_norm(h, (C,), t[p + ".block.2.weight"], t[p + ".block.2.bias"], 1e-5)
                h = F.gelu(F.linear(h, t[p + ".block.3.weight"], t[p + ".block.3.bias"]), approximate="tanh")
                h = F.linear(h, t[p + ".block.5.weight"], t[p + ".block.5.bias"]).permute(0, 3, 1, 2)
                r = h * t[p + ".layer_scale"]
                if masks is not None and masks[0][bi] is not None:
                    r = r * torch.stack([torch.from_numpy(m[bi]) for m in masks]).to(device).reshape(x.shape[0], C, 1, 1)
                x = x + r
                bi += 1
        v = x.mean((2, 3))
        v = F.layer_norm(v, (v.shape[1],), t["classifier.0.weight"], t["classifier.0.bias"], 1e-6)
        return F.linear(v, t["classifier.2.weight"], t["classifier.2.bias"]).cpu().numpy()


def training_masks(setting, keys, p):
    """Per sample (keys uint32 [B, 2]): the per-block DropPath scales of a training-mode forward at stochastic_depth_prob p."""
    probs = _sd_probs(p, setting)
    return [_masks(_block_keys(k, setting), probs, _widths(setting)) for k in np.asarray(keys, np.uint32)]
