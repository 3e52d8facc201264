"""numpy reference of the mixed-precision Conv2d (csrc/conv_mp.hip; filter_value_and_grad(..., conv_dtype="bf16")): float64 references
of the three products on r(.) operands (r = tests/_linear_mp_ref.rne_bf16), the same contractions on absolute values, the generators of
the cases of tests/test_conv_mp_gpu.py (proved on the CPU by tests/test_conv_mp_host.py), the entry's wgrad split arithmetic restated
from its comment, and the model emulation.

Maps NHWC, filters KRSC, groups = 1.  in(p, r, s) = (n, ho sh - ph + r dh, wo sw - pw + s dw), zeros outside the map.
    fwd    y [p,k]     = sum r(x[in(p,r,s),c]) r(w[k,r,s,c]) + bias[k]       reduction R S C     (the bias is NOT rounded)
    dgrad  dx[q,c]     = sum over k and the taps whose stride divides, of r(dy[out(q,r,s),k]) r(w[k,r,s,c])
    wgrad  dw[k,r,s,c] = sum over p of r(dy[p,k]) r(x[in(p,r,s),c])          reduction P = N Ho Wo

The references walk the taps the way the kernels do (a gather per tap with a validity mask), so that the defects a kernel can have --
a missing stride test, swapped taps, an ignored dilation, a dropped ragged chunk of positions -- can be put in by name (`defect`)."""
import functools

import numpy as np

from tests import _strict as S
from tests._linear_mp_ref import _cover, _ties, prove_round_core, rne_bf16, wgrad_split_rule

F64 = np.float64
ENTRIES = ("fwd", "dgrad", "wgrad")
TILE, KSTEP = 128, 32                 # the kernel's tile edge and reduction step (LMP_T, LMP_S): the issue's shapes need no analogues
DEFECTS = ("dgrad_no_stride_test", "taps_transposed", "dilation_ignored", "wgrad_drops_ragged_chunk")

# (N, H, W, C, K, (R, S), stride, pad, dil): the issue's nine shapes
_SHAPES = [
    (1, 1, 1, 1, 1, (1, 1), 1, 0, 1),                 # 1 a tile that is all edge
    (1, 5, 5, 3, 8, (3, 3), 1, 1, 1),                 # 2 C = 3: 4-byte loads, a channel chunk that is almost all padding
    (2, 9, 7, 16, 24, (3, 3), 2, 1, 1),               # 3 stride 2 on an odd map: dgrad's "stride divides" rule
    (1, 8, 8, 40, 130, (3, 3), 1, 2, 2),              # 4 dilation 2, a ragged second channel chunk, a second output-column tile of 2
    (1, 9, 12, 8, 8, (1, 7), (2, 1), (0, 3), 1),      # 5 R != S, sh != sw, ph != pw
    (2, 12, 12, 33, 17, (7, 7), 2, 3, 1),             # 6 stem-like, odd C and K: every operand on the unaligned path
    (1, 6, 6, 64, 64, (1, 1), 2, 0, 1),               # 7 the strided pointwise shortcut, not a Linear
    (3, 11, 11, 32, 32, (3, 3), 1, 1, 1),             # 8 363 positions: three row tiles, the last ragged; tile rows cross images
    (3, 5, 3, 16, 40, (3, 3), 1, 0, 1),               # 9 Wo = 1, P = 9
]
SHAPES = [S.ConvGeom(*s, 1) for s in _SHAPES]
BOUND_SHAPES = SHAPES + [S.ConvGeom(2, 14, 14, 256, 256, (3, 3), 1, 1, 1, 1)]
# the shape whose weight gradient wants more than two parts: P = 3 * 17 * 16 = 816 -> 26 steps -> 3 parts of 288, the last ragged (240)
SPLIT_SHAPE = S.ConvGeom(3, 17, 16, 8, 8, (3, 3), 1, 1, 1, 1)
# the rounding-visible shapes: reduction 16 each (R S C = 2 2 4; K x taps = 4 x 4; P = 4 x 4)
ROUND_SHAPES = {"fwd": S.ConvGeom(1, 6, 6, 4, 33, (2, 2), 1, 0, 1, 1), "dgrad": S.ConvGeom(1, 6, 6, 33, 4, (2, 2), 1, 0, 1, 1),
                "wgrad": S.ConvGeom(1, 5, 5, 33, 5, (2, 2), 1, 0, 1, 1)}


def identity(a):
    return np.asarray(a, np.float32)


def args_of(g):
    """The entries' argument tail: N, H, W, C, K, R, S, sh, sw, ph, pw, dh, dw (no groups)."""
    return g.args()[:-1]


def out_shape(entry, g):
    return {"fwd": (g.N, g.Ho, g.Wo, g.K), "dgrad": (g.N, g.H, g.W, g.C), "wgrad": (g.K, g.R, g.S, g.C)}[entry]


def kred_of(entry, g):
    return {"fwd": g.R * g.S * g.C, "dgrad": g.K * g.R * g.S, "wgrad": g.P}[entry]


# ------------------------------------------------------------------------------------------------ float64 references
def _tap_offsets(g, r, s, defect):
    """The (h, w) offsets of tap (r, s) in input pixels."""
    dh, dw = (1, 1) if defect == "dilation_ignored" else (g.dh, g.dw)
    if defect == "taps_transposed":
        r, s = s, r
    return r * dh, s * dw


def _gather_x(x, g, r, s, defect=None):
    """x[in(p, r, s), :] for every output position: [N, Ho, Wo, C], zeros in the padding."""
    oh, ow = _tap_offsets(g, r, s, defect)
    hi, wi = np.arange(g.Ho) * g.sh - g.ph + oh, np.arange(g.Wo) * g.sw - g.pw + ow
    vh, vw = (hi >= 0) & (hi < g.H), (wi >= 0) & (wi < g.W)
    patch = x[:, np.clip(hi, 0, g.H - 1)][:, :, np.clip(wi, 0, g.W - 1)]
    return patch * (vh[:, None] & vw[None, :])[None, :, :, None]


def _gather_dy(dy, g, r, s, defect=None):
    """dy[out(q, r, s), :] for every input position: [N, H, W, K], zeros where the tap does not reach an output position."""
    oh, ow = _tap_offsets(g, r, s, defect)
    u, v = np.arange(g.H) + g.ph - oh, np.arange(g.W) + g.pw - ow
    ho, wo = u // g.sh, v // g.sw
    vh, vw = (u >= 0) & (ho < g.Ho), (v >= 0) & (wo < g.Wo)
    if defect != "dgrad_no_stride_test":
        vh, vw = vh & (u % g.sh == 0), vw & (v % g.sw == 0)
    patch = dy[:, np.clip(ho, 0, g.Ho - 1)][:, :, np.clip(wo, 0, g.Wo - 1)]
    return patch * (vh[:, None] & vw[None, :])[None, :, :, None]


def _contract(entry, g, x, w, dy, defect):
    if entry == "fwd":
        y = np.zeros((g.N, g.Ho, g.Wo, g.K), F64)
        for r in range(g.R):
            for s in range(g.S):
                y += _gather_x(x, g, r, s, defect) @ w[:, r, s, :].T
        return y
    if entry == "dgrad":
        dx = np.zeros((g.N, g.H, g.W, g.C), F64)
        for r in range(g.R):
            for s in range(g.S):
                dx += _gather_dy(dy, g, r, s, defect) @ w[:, r, s, :]
        return dx
    dw = np.zeros((g.K, g.R, g.S, g.C), F64)
    keep = g.P // KSTEP * KSTEP if defect == "wgrad_drops_ragged_chunk" else g.P
    d2 = dy.reshape(g.P, g.K)[:keep]
    for r in range(g.R):
        for s in range(g.S):
            dw[:, r, s, :] = d2.T @ _gather_x(x, g, r, s, defect).reshape(g.P, g.C)[:keep]
    return dw


def product_ref(entry, g, x=None, w=None, dy=None, bias=None, rnd=rne_bf16, rnd_bias=None, defect=None):
    """(ref, mag) in float64: the product of the ROUNDED operands (+ the un-rounded bias for the forward) and the same contraction on
    absolute values.  `rnd` / `rnd_bias` / `defect` let the host tests put a defective kernel in."""
    x, w, dy = (None if a is None else np.asarray(rnd(a), F64) for a in (x, w, dy))
    ab = lambda a: None if a is None else np.abs(a)
    ref, mag = _contract(entry, g, x, w, dy, defect), _contract(entry, g, ab(x), ab(w), ab(dy), defect)
    if entry == "fwd" and bias is not None:
        bb = np.asarray(bias if rnd_bias is None else rnd_bias(bias), F64)
        ref, mag = ref + bb, mag + np.abs(bb)
    return ref, mag


def weights_of(entry, g, x, w, dy):
    """The (rows, reduction) matrices S.prove_exact's coverage looks at."""
    if entry == "fwd":
        return [w.reshape(g.K, -1), x.reshape(-1, g.C)]
    if entry == "dgrad":
        return [w.transpose(3, 0, 1, 2).reshape(g.C, -1), dy.reshape(-1, g.K)]
    return [dy.reshape(-1, g.K).T, x.reshape(-1, g.C).T]


# ------------------------------------------------------------------------------------------------ case generators
def _shapes(g):
    return (g.N, g.H, g.W, g.C), (g.K, g.R, g.S, g.C), (g.N, g.Ho, g.Wo, g.K)


@functools.lru_cache(maxsize=None)
def int_case(g, seed=7):
    """x, w, dy, bias: integers in [-2, 2] (bf16 values); no all-zero pixel, channel, filter or tap column in any operand."""
    rng = S.rng_of(seed)
    xs, ws, ys = _shapes(g)
    x = _cover(S.int_tensor(rng, (g.N * g.H * g.W, g.C), 2), rng).reshape(xs)
    w = _cover(S.int_tensor(rng, (g.K, g.R * g.S * g.C), 2), rng)
    w = _cover(w.reshape(g.K * g.R * g.S, g.C), rng).reshape(ws)
    dy = _cover(S.int_tensor(rng, (g.P, g.K), 2), rng).reshape(ys)
    bias = S.int_tensor(rng, (g.K,), 2)
    return x, w, dy, bias


def _ties_any(rng, shape):
    """_ties for a tensor of any size: _ties plants its 256 ties over the first min(n, 256) elements, which leaves a tensor of fewer
    than that no value BESIDE a tie.  Below 1024 elements half of the tensor is planted instead, cyclically with the eight classes
    (tie of either parity, the value just below / above a tie) x (both signs); the other half stays the random draw of k 2^-10."""
    n = int(np.prod(shape))
    if n >= 1024:
        return _ties(rng, shape)
    k = rng.integers(512, 2048, n) * rng.choice([-1, 1], n)
    ties = np.arange(1024 + 4, 2048, 8)
    even, odd = ties[((ties >> 3) & 1) == 0], ties[((ties >> 3) & 1) == 1]
    m = n // 2
    classes = [even, odd, ties - 1, ties + 1]
    planted = np.array([rng.choice(classes[(i // 2) % 4]) * (1 if i % 2 else -1) for i in range(m)])
    k[:m] = planted
    k = k[rng.permutation(n)]
    return (k.astype(F64) * 2.0 ** -10).astype(np.float32).reshape(shape)


@functools.lru_cache(maxsize=None)
def round_case(entry, seed=11):
    """Operands k 2^-10 with every tie class planted (_ties / _ties_any); bias an odd multiple of 2^-16 with |bias| <= 32 that is NOT a bf16 value."""
    g = ROUND_SHAPES[entry]
    rng = S.rng_of(seed)
    xs, ws, ys = _shapes(g)
    x, w, dy = _ties_any(rng, xs), _ties_any(rng, ws), _ties_any(rng, ys)
    kb = rng.integers(-(32 << 16) // 2, (32 << 16) // 2, g.K) * 2 + 1
    kb[np.abs(kb) < 1024] += 4096
    bias = (kb.astype(F64) * 2.0 ** -16).astype(np.float32)
    return x, w, dy, bias


@functools.lru_cache(maxsize=None)
def gauss_case(g, seed=13):
    rng = S.rng_of(seed)
    xs, ws, ys = _shapes(g)
    x = rng.standard_normal(xs).astype(np.float32)
    w = (rng.standard_normal(ws) / np.sqrt(g.R * g.S * g.C)).astype(np.float32)
    dy = rng.standard_normal(ys).astype(np.float32)
    bias = (0.1 * rng.standard_normal(g.K)).astype(np.float32)
    return x, w, dy, bias


def operands_of(entry, x, w, dy):
    return {"fwd": (x, w), "dgrad": (dy, w), "wgrad": (dy, x)}[entry]


def prove_round_case(entry, g, ref, mag, x, w, dy, bias):
    """_linear_mp_ref.prove_round_core on this entry's operands, for a reduction of 16."""
    assert kred_of(entry, g) == 16
    prove_round_core("conv_mp", entry, ref, mag, weights_of(entry, g, x, w, dy), operands_of(entry, x, w, dy), bias)


# ------------------------------------------------------------------------------------------------ wgrad's split
def wgrad_split(g, offer=None):
    """mv_conv2d_mp_wgrad: one tile per (128 filters, tap, 128 channels) of dw [K, R, S, C], the reduction runs over the P positions."""
    return wgrad_split_rule(-(-g.K // TILE) * g.R * g.S * -(-g.C // TILE), g.P, g.out_elems, offer)


# ------------------------------------------------------------------------------------------------ the rule
def rule_ref(g, x, w, bias, res, gy):
    """g_conv2d under "bf16" with bias + residual + relu in float64: y = relu(z), z = conv(r(x), r(w)) + bias + res; g2 = gy [z > 0].
    Returns {"y": (ref, mag of z), "z", "g2"}; dx, dW and db are referred to the DEVICE's g2 by the test (each product held to its own bound)."""
    z, zmag = product_ref("fwd", g, x=x, w=w, bias=bias)
    z, zmag = z + np.asarray(res, F64), zmag + np.abs(np.asarray(res, F64))
    return {"y": (np.maximum(z, 0.0), zmag), "z": z, "g2": np.asarray(gy, F64) * (z > 0)}


# ------------------------------------------------------------------------------------------------ the model case (resnet18)
RESNET_CLASSES, RESNET_B, RESNET_SIZE = 5, 2, 32


@functools.lru_cache(maxsize=None)
def resnet_refs():
    """resnet18, 32 x 32, 5 classes, B = 2, inference-mode BatchNorm on oracle/torch_grad.resnet (imported, not edited): "a" = (loss, grads)
    in float64 as it is; "b" = float64 with torch.nn.functional.conv2d replaced, for the duration of the call, by an autograd Function that
    rounds x, w and the incoming gradient with rne_bf16 (of their fp32 values) for groups == 1; the bias gradient is the un-rounded one."""
    import torch

    from oracle import state as ST
    from oracle import torch_grad as TG
    block, layers = "basic", (2, 2, 2, 2)
    sd = ST.resnet_state(1, block, layers, RESNET_CLASSES)
    x = ST.synthetic_images(RESNET_B, RESNET_SIZE, seed=5)
    labels = np.arange(RESNET_B) % RESNET_CLASSES
    orig = torch.nn.functional.conv2d

    def r(t):
        return torch.from_numpy(rne_bf16(t.detach().to(torch.float32).numpy()).astype(F64))

    class RoundedConv(torch.autograd.Function):
        @staticmethod
        def forward(ctx, xx, w, b, stride, padding, dilation):
            xr, wr = r(xx), r(w)
            ctx.save_for_backward(xr, wr)
            ctx.geom = (stride, padding, dilation)
            ctx.has_bias = b is not None
            return orig(xr, wr, b, stride, padding, dilation, 1)

        @staticmethod
        def backward(ctx, gg):
            xr, wr = ctx.saved_tensors
            stride, padding, dilation = ctx.geom
            gr = r(gg)
            dx = torch.nn.grad.conv2d_input(xr.shape, wr, gr, stride, padding, dilation, 1)
            dw = torch.nn.grad.conv2d_weight(xr, wr.shape, gr, stride, padding, dilation, 1)
            db = gg.sum((0, 2, 3)) if ctx.has_bias else None
            return dx, dw, db, None, None, None

    def patched(xx, w, b=None, stride=1, padding=0, dilation=1, groups=1):
        if groups != 1:
            return orig(xx, w, b, stride, padding, dilation, groups)
        return RoundedConv.apply(xx, w, b, stride, padding, dilation)

    a = TG.resnet(sd, x, labels, block, layers, dtype=torch.float64)
    torch.nn.functional.conv2d = patched
    try:
        b = TG.resnet(sd, x, labels, block, layers, dtype=torch.float64)
    finally:
        torch.nn.functional.conv2d = orig
    names = [k for k in sd if k in a[1]]
    return {"sd": sd, "x": x, "labels": labels, "a": a, "b": b, "names": names}
