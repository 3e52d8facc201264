"""Swin Transformer V2 restated literally in float64 torch (reference models/classification/swin.py: `_PatchMergingV2` :68-87,
`_shifted_window_attention` with logit_scale :90-255, `_ShiftedWindowAttentionV2` :369-522, `_SwinTransformerBlockV2` :581-635,
`SwinTransformer.__call__` :760-772).  Independent of the package: weights come in as plain dicts of arrays (`weights_of` reads them
off a model tree by attribute name only).  The reference's quirks are kept as data: the index is relative_coords.sum(-1) with
negative values wrapping, the cpb_mlp output (heads, 2Wh-1, 2Ww-1) is reshaped RAW to (-1, heads), q and k are normalised over
axis 0 = the windows of one image, and the key third of the qkv bias is zeroed on every call.

`emulate="bf16"` rounds (to nearest even) where the engine's bf16 mode rounds: the operands of every GEMM (the stream's bf16 plane,
the weights unless `precise(C, depth)` says the layer runs with split-precision weights, qkv, the hidden activations), q_hat and
k_hat after an fp32 product with the fp32 reciprocal norm, the un-normalised probabilities P, and the attention output.  The
deviation of that run from the float64 run measures the reference's own sensitivity to bf16 rounding (test_swin_v2_gpu.py).
"""
from __future__ import annotations

import math

import numpy as np
import torch

F64 = torch.float64


def t64(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64)))


def bf(x):
    """Round to bf16 (nearest even), back in float64."""
    return x.to(torch.float32).to(torch.bfloat16).to(F64)


def f32(x):
    return x.to(torch.float32).to(F64)


# ------------------------------------------------------------------------------------------------ tables (:435-484)
def coords_table(window):
    wh, ww = window
    rh = np.arange(-(wh - 1), wh, dtype=np.float64)
    rw = np.arange(-(ww - 1), ww, dtype=np.float64)
    t = np.stack(np.meshgrid(rh, rw, indexing="ij")).transpose(1, 2, 0)
    t = np.stack([t[:, :, 0] / wh - 1, t[:, :, 1] / ww - 1], axis=-1)
    t = 8 * t
    return np.sign(t) * np.log2(np.abs(t) + 1.0) / 3.0


def rel_index(window):
    wh, ww = window
    coords = np.stack(np.meshgrid(np.arange(wh), np.arange(ww), indexing="ij")).reshape(2, -1)
    rel = (coords[:, :, None] - coords[:, None, :]).transpose(1, 2, 0)
    return rel.sum(-1).reshape(-1)


def _cpb(table, w1, b1, w2):
    """cpb_mlp (:418-426) -> (heads, 2Wh-1, 2Ww-1)."""
    t = np.asarray(table, np.float64).transpose(2, 0, 1)                        # Lambda(transpose (2, 0, 1))
    h = np.einsum("oc,chw->ohw", np.asarray(w1, np.float64), t) + np.asarray(b1, np.float64).reshape(-1, 1, 1)
    h = np.maximum(h, 0.0)
    return np.einsum("oc,chw->ohw", np.asarray(w2, np.float64), h)              # Lambda(transpose (0, 1, 2)): the identity


def rel_bias(table, index, w1, b1, w2, heads, window):
    """get_relative_position_bias (:486-495): raw reshape, wrap-around gather, 16 sigmoid."""
    n = window[0] * window[1]
    raw = _cpb(table, w1, b1, w2).reshape(-1, heads)
    b = raw[np.asarray(index).reshape(-1).astype(np.int64)].reshape(n, n, -1).transpose(2, 0, 1)
    return 16.0 / (1.0 + np.exp(-b))


def rel_bias_transposed(table, index, w1, b1, w2, heads, window):
    """What a torchvision-style reading would give: positions-major (P, heads) = the TRANSPOSE of the MLP output."""
    n = window[0] * window[1]
    raw = _cpb(table, w1, b1, w2).reshape(heads, -1).T
    b = raw[np.asarray(index).reshape(-1).astype(np.int64)].reshape(n, n, -1).transpose(2, 0, 1)
    return 16.0 / (1.0 + np.exp(-b))


# ------------------------------------------------------------------------------------------------ windows (:106-141, :235-255)
def eff_shift(H, W, window, shift):
    return [0 if window[0] >= H else shift[0], 0 if window[1] >= W else shift[1]]


def partition(x, window, shift):
    """x (H, W, C) -> (nW, n, C) after the cyclic shift."""
    H, W, C = x.shape
    s = eff_shift(H, W, window, shift)
    if sum(s) > 0:
        x = torch.roll(x, shifts=(-s[0], -s[1]), dims=(0, 1))
    x = x.reshape(H // window[0], window[0], W // window[1], window[1], C)
    return x.permute(0, 2, 1, 3, 4).reshape(-1, window[0] * window[1], C)


def reverse(x, H, W, window, shift):
    C = x.shape[-1]
    s = eff_shift(H, W, window, shift)
    x = x.reshape(H // window[0], W // window[1], window[0], window[1], C).permute(0, 2, 1, 3, 4).reshape(H, W, C)
    if sum(s) > 0:
        x = torch.roll(x, shifts=(s[0], s[1]), dims=(0, 1))
    return x


def shift_mask(H, W, window, shift):
    """(nW, n, n) of 0 / -100 (:175-217), or None."""
    s = eff_shift(H, W, window, shift)
    if sum(s) == 0:
        return None
    m = torch.zeros(H, W, dtype=F64)
    hs = ((0, H - window[0]), (H - window[0], H - s[0]), (H - s[0], H))
    ws = ((0, W - window[1]), (W - window[1], W - s[1]), (W - s[1], W))
    c = 0
    for h0, h1 in hs:
        for w0, w1 in ws:
            m[h0:h1, w0:w1] = c
            c += 1
    m = m.reshape(H // window[0], window[0], W // window[1], window[1]).permute(0, 2, 1, 3).reshape(-1, window[0] * window[1])
    d = m[:, None, :] - m[:, :, None]
    return torch.where(d == 0, 0.0, -100.0).to(F64)


def rnorm_windows(x):
    """1 / jnp.linalg.norm(x, ord=2, axis=0) for x (nW, ...)."""
    return 1.0 / torch.sqrt((x * x).sum(0))


def cos_logits(q, k, logit_scale):
    """(:159-168) q, k (nW, heads, n, dh); logit_scale (heads, 1, 1)."""
    a = (q / torch.linalg.norm(q, ord=2, dim=0)) @ (k / torch.linalg.norm(k, ord=2, dim=0)).transpose(-2, -1)
    return a * torch.exp(torch.clamp(logit_scale, max=math.log(100.0)))


def attention_core(qkv, bias, logit_scale, heads, window, shift, emulate=None, attn_mask=None, stats=None):
    """qkv (H, W, 3C) of ONE image -> (H, W, C): partition, cosine logits, bias, mask, softmax, [dropout mask], P V, reverse.
    attn_mask: (nW, heads, n, n) of {0, 1 / keep}.  stats: a list that receives (|q|, |k|) when the image has one window."""
    H, W, C3 = qkv.shape
    C = C3 // 3
    xw = partition(qkv, window, shift)
    nW, n, _ = xw.shape
    t = xw.reshape(nW, n, 3, heads, C // heads).permute(2, 0, 3, 1, 4)
    q, k, v = t[0], t[1], t[2]
    if nW == 1 and stats is not None:
        stats.append((q.abs().reshape(-1).clone(), k.abs().reshape(-1).clone()))
    mul = torch.exp(torch.clamp(logit_scale.reshape(heads, 1, 1), max=math.log(100.0)))
    if emulate == "bf16":
        rq, rk = f32(rnorm_windows(f32(q))), f32(rnorm_windows(f32(k)))
        qh, kh = bf(f32(q * rq)), bf(f32(k * rk))
        a = qh @ kh.transpose(-2, -1) * f32(mul)
    else:
        a = (q / torch.linalg.norm(q, ord=2, dim=0)) @ (k / torch.linalg.norm(k, ord=2, dim=0)).transpose(-2, -1) * mul
    a = a + bias
    m = shift_mask(H, W, window, shift)
    if m is not None:
        a = a + m[:, None]
    if emulate == "bf16":
        e = torch.exp(a - a.max(-1, keepdim=True).values)
        den = e.sum(-1, keepdim=True)
        if attn_mask is not None:
            e = e * attn_mask
        o = bf((bf(e) @ v) / den)
    else:
        p = torch.softmax(a, dim=-1)
        if attn_mask is not None:
            p = p * attn_mask
        o = p @ v
    o = o.permute(0, 2, 1, 3).reshape(nW, n, C)
    return reverse(o, H, W, window, shift)


# ------------------------------------------------------------------------------------------------ layers
def layernorm(x, g, b, eps=1e-5):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * g + b


def gelu_tanh(x):
    return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))


def _lin(x, w, b, emulate, split):
    if emulate == "bf16":
        x = bf(x)
        if not split:
            w = bf(w)
    y = x @ w.T
    return y if b is None else y + b


def attention(x, p, heads, window, shift, emulate=None, split=False, attn_mask=None, out_mask=None, stats=None):
    """`_ShiftedWindowAttentionV2.__call__` on x (H, W, C).  out_mask: (nW, n, C) of {0, 1 / keep}, the second _func_dropout."""
    H, W, C = x.shape
    bq = p["qkv.bias"].clone()
    bq[C:2 * C] = 0                                                             # :144-150
    qkv = _lin(x, p["qkv.weight"], bq, emulate, split)
    if emulate == "bf16":
        qkv = bf(qkv)
    bias = t64(rel_bias(p["table"], p["index"], p["cpb.w1"], p["cpb.b1"], p["cpb.w2"], heads, window))
    o = attention_core(qkv, bias, p["logit_scale"], heads, window, shift, emulate, attn_mask, stats)
    y = _lin(o, p["proj.weight"], p["proj.bias"], emulate, split)
    if out_mask is not None:
        y = reverse(partition(y, window, shift) * out_mask, H, W, window, shift)
    return y


def block(x, p, heads, window, shift, emulate=None, split=False, drop=None, stats=None):
    """`_SwinTransformerBlockV2.__call__` (:629-635).  drop: dict with optional 'attn' (nW, heads, n, n), 'proj' (nW, n, C),
    'sd1' / 'sd2' (C,) stochastic-depth scales (mode "local": one draw per channel of the (C, H, W) sample)."""
    drop = drop or {}
    a = layernorm(attention(x, p, heads, window, shift, emulate, split, drop.get("attn"), drop.get("proj"), stats), p["norm1.weight"],
                  p["norm1.bias"])
    if "sd1" in drop:
        a = a * drop["sd1"]
    x = x + a
    h = gelu_tanh(_lin(x, p["fc1.weight"], p["fc1.bias"], emulate, split))
    m = layernorm(_lin(h, p["fc2.weight"], p["fc2.bias"], emulate, split), p["norm2.weight"], p["norm2.bias"])
    if "sd2" in drop:
        m = m * drop["sd2"]
    return x + m


def patch_merging(x, p, emulate=None):
    """`_PatchMergingV2.__call__` (:83-87) on x (H, W, C), even sizes; the reduction runs with split-precision weights."""
    g = torch.cat([x[0::2, 0::2], x[1::2, 0::2], x[0::2, 1::2], x[1::2, 1::2]], dim=-1)
    return layernorm(_lin(g, p["reduction.weight"], None, emulate, True), p["norm.weight"], p["norm.bias"])


def model(x, P, emulate=None, precise=lambda C, depth: False, drops=None):
    """SwinTransformer with V2 blocks on ONE image x (3, H, W).  P: the dict of `weights_of`.  The patch embedding, the final norm,
    the pool and the head run in fp32 in the engine's bf16 mode: no rounding here.  drops: per block index, the dict of `block`.
    Returns (logits, stats) with stats the (|q|, |k|) of every single-window attention."""
    stats = []
    w = P["embed.weight"]
    y = torch.nn.functional.conv2d(x[None], w, P["embed.bias"].reshape(-1), stride=w.shape[-1])[0].permute(1, 2, 0)
    y = layernorm(y, P["embed.norm.weight"], P["embed.norm.bias"])
    bi = 0
    for si, st in enumerate(P["stages"]):
        for li, bp in enumerate(st["blocks"]):
            shift = [0, 0] if li % 2 == 0 else [v // 2 for v in P["window"]]
            y = block(y, bp, st["heads"], P["window"], shift, emulate, precise(y.shape[-1], len(st["blocks"])),
                      None if drops is None else drops.get(bi), stats)
            bi += 1
        if st.get("merge") is not None:
            y = patch_merging(y, st["merge"], emulate)
    y = layernorm(y, P["norm.weight"], P["norm.bias"]).mean(dim=(0, 1))
    return y @ P["head.weight"].T + P["head.bias"], stats


def weights_of(m):
    """A SwinTransformer tree with V2 blocks -> the plain dict `model` reads (attribute names only)."""
    L = m.features.layers
    P = {"embed.weight": t64(L[0].layers[0].weight), "embed.bias": t64(L[0].layers[0].bias),
         "embed.norm.weight": t64(L[0].layers[1].weight), "embed.norm.bias": t64(L[0].layers[1].bias),
         "norm.weight": t64(m.norm.weight), "norm.bias": t64(m.norm.bias), "head.weight": t64(m.head.weight),
         "head.bias": t64(m.head.bias), "stages": []}
    i = 1
    while i < len(L):
        blocks = []
        for b in L[i].layers:
            a = b.attn
            lins = [l for l in a.cpb_mlp.layers if hasattr(l, "weight")]
            P["window"] = list(a.window_size)
            blocks.append({"qkv.weight": t64(a.qkv.weight), "qkv.bias": t64(a.qkv.bias), "proj.weight": t64(a.proj.weight),
                           "proj.bias": t64(a.proj.bias), "logit_scale": t64(a.logit_scale), "table": np.asarray(a.relative_position_bias_table),
                           "index": np.asarray(a.relative_position_index), "cpb.w1": np.asarray(lins[0].weight),
                           "cpb.b1": np.asarray(lins[0].bias), "cpb.w2": np.asarray(lins[1].weight),
                           "norm1.weight": t64(b.norm1.weight), "norm1.bias": t64(b.norm1.bias), "norm2.weight": t64(b.norm2.weight),
                           "norm2.bias": t64(b.norm2.bias), "fc1.weight": t64(b.mlp.fc1.weight), "fc1.bias": t64(b.mlp.fc1.bias),
                           "fc2.weight": t64(b.mlp.fc2.weight), "fc2.bias": t64(b.mlp.fc2.bias)})
        st = {"blocks": blocks, "heads": L[i].layers[0].attn.num_heads, "merge": None}
        i += 1
        if i < len(L):
            st["merge"] = {"reduction.weight": t64(L[i].reduction.weight), "norm.weight": t64(L[i].norm.weight),
                           "norm.bias": t64(L[i].norm.bias)}
            i += 1
        P["stages"].append(st)
    return P
