"""numpy reference of the mixed-precision Linear (csrc/linear_mp.hip; filter_value_and_grad(..., matmul_dtype="bf16")): the rounding
r(.) = fp32 -> bf16 round-to-nearest-even, float64 references of the three products on r(.) operands and of the rule, and the
generators of the cases of tests/test_linear_mp_gpu.py (proved on the CPU by tests/test_linear_mp_host.py).

    fwd    y [M,N] = r(x[M,K]) . r(w[N,K])^T + bias      reduction K     (the bias is NOT rounded)
    dgrad  dx[M,K] = r(g[M,N]) . r(w[N,K])               reduction N
    wgrad  dw[N,K] = r(g[M,N])^T . r(x[M,K])             reduction M
"""
import functools

import numpy as np

from tests import _strict as S

F64 = np.float64
ENTRIES = ("fwd", "dgrad", "wgrad")
TILE, KSTEP = 128, 32                 # the kernel's tile edge and reduction step (LMP_T, LMP_S)

# (M, N, K): the issue's list, then (T + 1, T + 2, S + 1) and (2 T, T, 2 S)
SHAPES = [(1, 1, 1), (33, 17, 9), (64, 128, 16), (130, 129, 65), (257, 96, 40), (TILE + 1, TILE + 2, KSTEP + 1), (2 * TILE, TILE, 2 * KSTEP)]
BOUND_SHAPES = SHAPES + [(788, 192, 768)]


def shape_id(s):
    return "x".join(str(v) for v in s)


# ------------------------------------------------------------------------------------------------ the rounding
def rne_bf16(a):
    """fp32 -> the nearest bf16 value (ties to the even bf16 mantissa), returned as fp32; integer arithmetic on the bit pattern.
    (Finite operands only: the carry of a rounding-up mantissa moves into the exponent, as it should.)"""
    u = np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32).reshape(np.shape(a))


def trunc_bf16(a):
    """Defect: the low 16 bits dropped."""
    u = np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32) & np.uint32(0xFFFF0000)
    return u.view(np.float32).reshape(np.shape(a))


def half_away_bf16(a):
    """Defect: ties go away from zero (add half an ulp of the magnitude, truncate)."""
    u = np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32).astype(np.uint64)
    u = (u + 0x8000) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32).reshape(np.shape(a))


def identity(a):
    """Defect: no rounding at all (fp32 products)."""
    return np.asarray(a, np.float32)


# ------------------------------------------------------------------------------------------------ float64 references
def _operands(entry, x, w, g):
    """(A, B) with the product A . B^T and the reduction along the last axis of both."""
    if entry == "fwd":
        return x, w
    if entry == "dgrad":
        return g, w.T
    return g.T, x.T


def product_ref(entry, x=None, w=None, g=None, bias=None, rnd=rne_bf16, rnd_bias=None):
    """(ref, mag) in float64: the product of the ROUNDED operands (+ the un-rounded bias for the forward) and the sum of the absolute
    values of its terms.  `rnd` / `rnd_bias` let the host tests put a defective rounding in."""
    a, b = _operands(entry, x, w, g)
    a, b = np.asarray(rnd(a), F64), np.asarray(rnd(b), F64)
    ref, mag = a @ b.T, np.abs(a) @ np.abs(b).T
    if entry == "fwd" and bias is not None:
        bb = np.asarray(bias if rnd_bias is None else rnd_bias(bias), F64)
        ref, mag = ref + bb, mag + np.abs(bb)
    return ref, mag


def kred_of(entry, M, N, K):
    return {"fwd": K, "dgrad": N, "wgrad": M}[entry]


def out_shape(entry, M, N, K):
    return {"fwd": (M, N), "dgrad": (M, K), "wgrad": (N, K)}[entry]


def act64(z, act):
    if act == "gelu":
        return S.act64(z, "gelu_tanh")
    return z


def rule_ref(x, w, bias, res, act, gy):
    """The rule of g_linear under "bf16" in float64: y = act(r(x) r(w)^T + bias + res); from the output gradient gy: g2 = gy act'(.) in
    float64, then dx = r(g2_32) r(w), dW = r(g2_32)^T r(x), db = colsum(g2_32), with g2_32 = fp32(g2): the gradient the products round is
    the fp32 tensor the backward holds.  Returns a dict of (ref, mag) pairs and the pre-activation."""
    z, zmag = product_ref("fwd", x=x, w=w, bias=bias)
    if res is not None:
        z, zmag = z + np.asarray(res, F64), zmag + np.abs(np.asarray(res, F64))
    y = act64(z, act)
    g2 = np.asarray(gy, F64) * (S.act_grad64(z, "gelu_tanh") if act == "gelu" else 1.0)
    g32 = g2.astype(np.float32)
    dx = product_ref("dgrad", w=w, g=g32)
    dw = product_ref("wgrad", x=x, g=g32)
    db = (g2.sum(0), np.abs(g2).sum(0))
    return {"y": (y, zmag), "dx": dx, "dw": dw, "db": db, "z": z, "g2": g2}


# ------------------------------------------------------------------------------------------------ case generators
def _cover(a, rng):
    """No all-zero row and no all-zero column (S.prove_exact's coverage of a weight matrix): a zero line gets one +-1."""
    a = a.copy()
    for r in np.flatnonzero(~(a != 0).any(axis=1)):
        a[r, rng.integers(0, a.shape[1])] = rng.choice([-1.0, 1.0])
    for c in np.flatnonzero(~(a != 0).any(axis=0)):
        a[rng.integers(0, a.shape[0]), c] = rng.choice([-1.0, 1.0])
    return a.astype(np.float32)


@functools.lru_cache(maxsize=None)
def int_case(M, N, K, seed=7):
    """x [M,K], w [N,K], g [M,N], bias [N]: integers in [-2, 2] (bf16 values), every row and column of every operand used."""
    rng = S.rng_of(seed)
    x, w, g = (_cover(S.int_tensor(rng, s, 2), rng) for s in ((M, K), (N, K), (M, N)))
    bias = S.int_tensor(rng, (N,), 2)
    return x, w, g, bias


def _ties(rng, shape):
    """k 2^-10 with |k| in [512, 2047] (magnitudes in [0.5, 2)): in [1, 2) the bf16 spacing is 2^-7 = 8 steps of k, so k % 8 == 4 is an
    exact tie; every tie of both parities (the neighbour below even / odd) and of both signs is planted, cyclically, over the first
    elements, and the values just beside the ties (k % 8 in {3, 5}) follow from the random draw."""
    n = int(np.prod(shape))
    k = rng.integers(512, 2048, n)
    ties = np.arange(1024 + 4, 2048, 8)                       # 128 ties: (k >> 3) & 1 alternates -> both parities
    planted = np.concatenate([ties, -ties])
    m = min(n, planted.size)
    k = k * rng.choice([-1, 1], n)
    k[:m] = planted[rng.permutation(planted.size)[:m]]
    k = k[rng.permutation(n)]
    return (k.astype(F64) * 2.0 ** -10).astype(np.float32).reshape(shape)


ROUND_RED = 16                # reduction length of the rounding-visible cases
ROUND_DIMS = (130, 33)


def round_shape(entry):
    """(M, N, K): the reduction length is 16, the other two dimensions 130 and 33."""
    a, b = ROUND_DIMS
    return {"fwd": (a, b, ROUND_RED), "dgrad": (a, ROUND_RED, b), "wgrad": (ROUND_RED, a, b)}[entry]


@functools.lru_cache(maxsize=None)
def round_case(entry, seed=11):
    """Operands k 2^-10 (see _ties); bias an integer multiple of 2^-16 with |bias| <= 32 that is NOT a bf16 value (odd multiples of
    2^-16 above 2^-8 need more than 8 significant bits)."""
    M, N, K = round_shape(entry)
    rng = S.rng_of(seed)
    x, w, g = _ties(rng, (M, K)), _ties(rng, (N, K)), _ties(rng, (M, N))
    kb = rng.integers(-(32 << 16) // 2, (32 << 16) // 2, N) * 2 + 1              # odd
    kb[np.abs(kb) < 1024] += 4096
    bias = (kb.astype(F64) * 2.0 ** -16).astype(np.float32)
    return x, w, g, bias


@functools.lru_cache(maxsize=None)
def gauss_case(M, N, K, seed=13):
    rng = S.rng_of(seed)
    x = rng.standard_normal((M, K)).astype(np.float32)
    w = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    g = rng.standard_normal((M, N)).astype(np.float32)
    bias = (0.1 * rng.standard_normal(N)).astype(np.float32)
    return x, w, g, bias


def prove_round_core(label, entry, ref, mag, weights, operands, bias):
    """The preconditions of a rounding-visible case (this file's and tests/_conv_mp_ref.py's), on the values times 2^16: integers below 2^24
    (S.prove_exact on `weights`, frac_bits = 16), both `operands` of magnitude in [0.5, 2) with every tie class present, the bias not a
    bf16 value."""
    S.prove_exact(f"{label}/{entry}/round", ref, mag, weights, out="fp32", frac_bits=16)
    for name, t in zip(("a", "b"), operands):
        k = np.rint(np.asarray(t, F64) * 1024).astype(np.int64)
        assert np.array_equal(k.astype(F64) * 2.0 ** -10, np.asarray(t, F64)) and (np.abs(k) >= 512).all() and (np.abs(k) <= 2047).all(), name
        tie = (np.abs(k) % 8 == 4) & (np.abs(k) >= 1024)
        par = (np.abs(k) >> 3) & 1
        for sign in (-1, 1):
            for p_ in (0, 1):
                assert (tie & (np.sign(k) == sign) & (par == p_)).any(), f"{entry}/{name}: no tie of sign {sign}, parity {p_}"
        assert (np.abs(k) % 8 == 3).any() and (np.abs(k) % 8 == 5).any(), f"{entry}/{name}: no value beside a tie"
        r = np.asarray(rne_bf16(t), F64) * 256
        assert np.array_equal(np.rint(r), r) and (np.abs(r) <= 512).all(), f"{entry}/{name}: rounded operand not a multiple of 2^-8 below 2"
    if entry == "fwd":
        assert (np.abs(bias) <= 32).all() and not np.array_equal(rne_bf16(bias), bias)
        assert (rne_bf16(bias) != bias).all(), "a bias element is a bf16 value"
    assert float(np.abs(mag).max()) < 2.0 ** 7


def prove_round_case(entry, ref, mag, x, w, g, bias):
    """prove_round_core on this entry's two operands (which are also the matrices S.prove_exact's coverage looks at)."""
    a, b = _operands(entry, x, w, g)
    prove_round_core("linear_mp", entry, ref, mag, [a, b], (a, b), bias)


# ------------------------------------------------------------------------------------------------ wgrad's split (linear_mp_tile.h)
def wgrad_split_rule(tiles, red, out_elems, offer=None):
    """(parts wanted, parts run with `offer` bytes of scratch, reduction elements per part): lmp_wgrad_split's rule for a weight gradient
    of `tiles` output tiles, reduction length `red` and `out_elems` outputs -- about 1024 workgroups, at least 8 steps of 32 per part, at
    most 64 parts, as many as the offer holds behind its first 4096 bytes, none below two; then no empty part."""
    steps = -(-red // KSTEP)
    want = 1 if tiles >= 1024 else -(-1024 // tiles)
    want = max(1, min(want, steps // 8, 64))
    split = want
    if split > 1:
        fit = 0 if offer is None else max(0, offer - 4096) // (out_elems * 4)
        split = 1 if fit < 2 else min(split, fit)
    chunk = -(-steps // split) * KSTEP
    return want, -(-red // chunk), chunk


def wgrad_split(M, N, K, offer=None):
    """mv_linear_mp_wgrad: 128 x 128 tiles of dw [N, K], the reduction runs over the M rows."""
    return wgrad_split_rule(-(-N // TILE) * -(-K // TILE), M, N * K, offer)


# ------------------------------------------------------------------------------------------------ the model case (vit)
VIT_CLASSES, VIT_B = 5, 2


@functools.lru_cache(maxsize=None)
def vit_refs():
    """vit 32 x 32, patch 8, width 64, depth 2, 2 heads, 5 classes, B = 2 on oracle/torch_grad.vit (imported, not edited):
    "a" = (loss, grads) in float64 as it is; "b" = float64 with torch.nn.functional.linear replaced, for the duration of the call, by
    an autograd Function that rounds x, w and the incoming gradient with rne_bf16 (of their fp32 values) -- every Linear but `fc`."""
    import torch

    from oracle import state as ST
    from oracle import torch_grad as TG
    sd = ST.vit_state(1, 32, 8, 64, 2, 2, 4, VIT_CLASSES)
    x = ST.synthetic_images(VIT_B, 32, seed=5)
    labels = np.arange(VIT_B) % VIT_CLASSES

    def r(t):
        return torch.from_numpy(rne_bf16(t.detach().to(torch.float32).numpy()).astype(F64))

    class RoundedLinear(torch.autograd.Function):
        @staticmethod
        def forward(ctx, xx, w, b):
            xr, wr = r(xx), r(w)
            ctx.save_for_backward(xr, wr)
            ctx.has_bias = b is not None
            y = xr @ wr.T
            return y if b is None else y + b

        @staticmethod
        def backward(ctx, g):
            xr, wr = ctx.saved_tensors
            gr = r(g)
            dx = gr @ wr
            dw = gr.reshape(-1, gr.shape[-1]).T @ xr.reshape(-1, xr.shape[-1])
            db = g.reshape(-1, g.shape[-1]).sum(0) if ctx.has_bias else None          # the bias gradient: the un-rounded gradient
            return dx, dw, db

    orig = torch.nn.functional.linear
    fc_shape = tuple(np.shape(sd["fc.weight"]))

    def patched(xx, w, b=None):
        if tuple(w.shape) == fc_shape:                    # the classifier head stays un-rounded
            return orig(xx, w, b)
        return RoundedLinear.apply(xx, w, b)

    a = TG.vit(sd, x, labels, 8, 2, 2, dtype=torch.float64)
    torch.nn.functional.linear = patched
    try:
        b = TG.vit(sd, x, labels, 8, 2, 2, dtype=torch.float64)
    finally:
        torch.nn.functional.linear = orig
    names = [k for k in sd if k in a[1]]
    return {"sd": sd, "x": x, "labels": labels, "a": a, "b": b, "names": names}
