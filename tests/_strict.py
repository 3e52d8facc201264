"""Strict parity instruments for the MFMA conv / GEMM kernels (used by test_strict_host.py and test_strict_gpu.py).

Instrument 1 -- exact integers.  Operands are small integers chosen so that every partial sum is an integer below 2^24 (exact in fp32
in ANY order: split-K, MFMA lane order) and everything stored as bf16 is an integer of magnitude <= 256 (exact in bf16).  The
kernel's output must then EQUAL the float64 reference; there is no tolerance.  `prove_exact` asserts those preconditions on the
CPU before anything is launched.

Instrument 2 -- per-element bound and rounding bias on Gaussian operands (bf16-rounded before both sides see them).  With
`mag` = the same contraction on absolute values (conv(|x|, |w|) |scale| + |shift| + |res|):

    e_pre = (K_red + 4) * 2^-23 * mag              fp32 accumulation in any order + 4 epilogue operations
    bound = e_pre + half_ulp_out(|ref| + e_pre)    half_ulp_out(v) = 2^(floor(log2 v) - 8) for bf16, 2^(floor(log2 v) - 24) for fp32

(activation none / ReLU: Lipschitz constant 1).  EVERY element must satisfy |got - ref| <= bound.  The rounding bias is
b = mean(sign(ref) (got - ref) / ulp_out(ref)) over the elements with |ref| >= 2^-6: round-to-nearest gives |b| ~ 0.005 over 4096
elements, truncation gives -0.5; |b| <= 0.05 is required of at least 4096 elements.

The memory-bound kernels (element-wise, activation, channel scale / affine, casts, layouts, pools, resize, gathers and the small
backward kernels; tests/test_strict_mem_gpu.py) use the same two instruments.  Their bound counts fp32 roundings instead of a
reduction length: `ops_bound(ref, mag, n_ops, out) = n_ops 2^-23 mag + half_ulp_out(|ref| + n_ops 2^-23 mag)`, `n_ops` counted from
the kernel source next to each case.  The second half of this file holds the case data, the float64 references and a numpy/float32
emulation of each kernel's contract (fp32 arithmetic in the kernel's order, then a round-to-nearest-even store); every emulation
takes a switch for exactly one defect, which tests/test_strict_host.py turns on to prove that the instrument sees it.
"""
from __future__ import annotations

import numpy as np
import torch

from oracle import np_ops as O

F64 = np.float64
BF16_INT_MAX = 256            # every integer of magnitude <= 256 is a bf16 value
ACC_INT_MAX = 1 << 24         # every integer below 2^24 is an fp32 value
BIAS_MIN_ELEMS = 4096
BIAS_LIMIT = 0.05
BIAS_MAX_KRED = 1152


def bf(a):
    return O.bf16_round(np.asarray(a, np.float32))


def rng_of(seed):
    return np.random.Generator(np.random.PCG64(seed))


# ------------------------------------------------------------------------------------------------ operand generators
def int_tensor(rng, shape, lim):
    """Integers in [-lim, lim] as float32."""
    return rng.integers(-lim, lim + 1, shape).astype(np.float32)


def pm1_rows(rng, rows, kred, nnz):
    """(rows, kred) float32: every row has exactly `nnz` entries of +-1 at random reduction positions, and every reduction position
    is hit by at least one row (a cyclic walk over a random permutation supplies the first entries of each row)."""
    if nnz > kred:
        raise AssertionError(f"pm1_rows: nnz = {nnz} > reduction length {kred}")
    cover = -(-kred // rows)
    if cover > nnz:
        raise AssertionError(f"pm1_rows: {rows} rows x nnz = {nnz} cannot cover a reduction of {kred}")
    perm = rng.permutation(kred)
    w = np.zeros((rows, kred), np.float32)
    for r in range(rows):
        pos = perm[(r * cover + np.arange(cover)) % kred]
        if nnz > cover:
            free = np.setdiff1d(np.arange(kred), pos, assume_unique=False)
            pos = np.concatenate([pos, rng.choice(free, nnz - cover, replace=False)])
        w[r, pos] = rng.choice(np.array([-1.0, 1.0], np.float32), pos.size)
    return w


def int_scale(rng, n, mags=(1, 2)):
    """BatchNorm scales in {+-1, +-2}; negatives included (every 5th at least, as the chain cases do)."""
    s = rng.choice(np.array(mags, np.float32), n) * rng.choice(np.array([-1.0, 1.0], np.float32), n)
    s[::5] = -np.abs(s[::5])
    return s.astype(np.float32)


def gauss_scale(rng, n):
    s = rng.uniform(0.5, 1.5, n).astype(np.float32)
    s[::5] *= -1.0
    return s


# ------------------------------------------------------------------------------------------------ float64 references
def _t(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, F64)))


def _conv64(x_nhwc, w_krsc, stride, pad, dil, groups):
    y = torch.nn.functional.conv2d(_t(x_nhwc).permute(0, 3, 1, 2), _t(w_krsc).permute(0, 3, 1, 2), None, stride, pad, dil, groups)
    return y.permute(0, 2, 3, 1).contiguous().numpy()


def epilogue64(acc, amag, scale, shift, res, act):
    """(ref, mag) of act(acc * scale + shift + res) with the channel last; `amag` is the contraction of the absolute values."""
    ref, mag = acc, amag
    if scale is not None:
        ref = ref * np.asarray(scale, F64)
        mag = mag * np.abs(np.asarray(scale, F64))
    if shift is not None:
        ref = ref + np.asarray(shift, F64)
        mag = mag + np.abs(np.asarray(shift, F64))
    if res is not None:
        ref = ref + np.asarray(res, F64)
        mag = mag + np.abs(np.asarray(res, F64))
    if act == 1:
        ref = np.maximum(ref, 0.0)
    elif act != 0:
        raise ValueError("strict instruments cover activation none / ReLU only")
    return ref, mag


def conv_ref(x_nhwc, w_krsc, scale, shift, res, act, stride=1, pad=0, dil=1, groups=1):
    acc = _conv64(x_nhwc, w_krsc, stride, pad, dil, groups)
    amag = _conv64(np.abs(x_nhwc), np.abs(w_krsc), stride, pad, dil, groups)
    return epilogue64(acc, amag, scale, shift, res, act)


def gemm_ref(x, w, scale, shift, res, act):
    x, w = np.asarray(x, F64), np.asarray(w, F64)
    return epilogue64(x @ w.T, np.abs(x) @ np.abs(w).T, scale, shift, res, act)


# ------------------------------------------------------------------------------------------------ instrument 1
def prove_exact(name, ref, mag, weights, stored=(), hidden=(), out="bf16", min_nonzero=0.10):
    """The exact-integer preconditions, asserted on the CPU before a launch (the float64 arrays hold integers far below 2^53, so the
    conversion to int64 is itself exact and checked):
      (a) `mag` (sum |x||w| * |scale| + |shift| + |res|) <= 256 for a bf16 output, and every operand in `stored` / intermediate in
          `hidden` is an integer of magnitude <= 256; mag < 2^24 for the fp32 accumulators;
      (b) every reduction index of every matrix in `weights` ((rows, reduction) layout) has a non-zero weight in some row, and every
          row has a non-zero weight;
      (c) fewer than 90 % of the reference outputs are zero."""
    for what, a in [("ref", ref), ("mag", mag)] + [(f"stored[{i}]", s) for i, s in enumerate(stored)] + \
                   [(f"hidden[{i}]", h) for i, h in enumerate(hidden)]:
        a = np.asarray(a, F64)
        ai = np.rint(a).astype(np.int64)
        assert np.array_equal(ai.astype(F64), a), f"{name}: {what} is not integer-valued"
        top = int(np.abs(ai).max()) if ai.size else 0
        assert top < ACC_INT_MAX, f"{name}: {what} reaches {top} >= 2^24 (fp32 accumulator not exact)"
        if out == "bf16" or what not in ("ref", "mag"):
            assert top <= BF16_INT_MAX, f"{name}: {what} reaches {top} > 256 (not exact in bf16)"
    for i, w in enumerate(weights):
        w2 = np.asarray(w).reshape(w.shape[0], -1) != 0
        assert w2.any(axis=0).all(), f"{name}: weights[{i}] leaves {int((~w2.any(axis=0)).sum())} reduction indices unused"
        assert w2.any(axis=1).all(), f"{name}: weights[{i}] has {int((~w2.any(axis=1)).sum())} all-zero output channels"
    zeros = float((np.asarray(ref) == 0).mean())
    assert zeros < 1.0 - min_nonzero, f"{name}: {100 * zeros:.1f} % of the reference outputs are zero (ReLU blanks the test)"


def check_exact(got, ref):
    """Bit equality of the values: np.array_equal, plus where the first differences are."""
    got, ref = np.asarray(got, F64), np.asarray(ref, F64)
    if got.shape != ref.shape:
        return {"ok": False, "err": f"shape {got.shape} vs {ref.shape}"}
    if np.array_equal(got, ref):
        return {"ok": True, "nbad": 0, "n": int(ref.size)}
    bad = np.argwhere(~(got == ref))
    ch = np.unique(bad[:, -1])
    return {"ok": False, "nbad": int(len(bad)), "n": int(ref.size), "maxdiff": float(np.nanmax(np.abs(got - ref))),
            "first": [(tuple(int(v) for v in b), float(got[tuple(b)]), float(ref[tuple(b)])) for b in bad[:6]],
            "bad_channels": [int(c) for c in ch[:32]], "n_bad_channels": int(ch.size)}


# ------------------------------------------------------------------------------------------------ instrument 2
def _exp(v):
    """floor(log2 v) for v > 0 (frexp: v = m 2^e, m in [0.5, 1))."""
    return np.frexp(v)[1] - 1


def half_ulp_out(v, out):
    v = np.asarray(v, F64)
    p = 8 if out == "bf16" else 24
    return np.where(v > 0, np.ldexp(1.0, _exp(np.where(v > 0, v, 1.0)) - p), 0.0)


def elem_bound(ref, mag, kred, out):
    e_pre = (kred + 4) * 2.0 ** -23 * np.asarray(mag, F64)
    return e_pre + half_ulp_out(np.abs(ref) + e_pre, out)


def ops_bound(ref, mag, n_ops, out):
    """`n_ops` fp32 roundings (2^-23 each, as in elem_bound) relative to `mag`, then the store's half ulp; n_ops may be an array."""
    e_pre = np.asarray(n_ops, F64) * 2.0 ** -23 * np.asarray(mag, F64)
    return e_pre + half_ulp_out(np.abs(np.asarray(ref, F64)) + e_pre, out)


def check_bound(got, ref, mag, kred, out, n_ops=None, bound=None):
    """Every element within elem_bound(kred) -- or, for the memory-bound kernels, within ops_bound(n_ops) (kred is then ignored), or
    within an explicit `bound` array."""
    got, ref = np.asarray(got, F64), np.asarray(ref, F64)
    if got.shape != ref.shape:
        return {"ok": False, "err": f"shape {got.shape} vs {ref.shape}"}
    if not np.isfinite(got).all():
        return {"ok": False, "err": "non-finite output", "nan": int((~np.isfinite(got)).sum())}
    if bound is not None:
        b = np.broadcast_to(np.asarray(bound, F64), ref.shape)
    else:
        b = elem_bound(ref, mag, kred, out) if n_ops is None else ops_bound(ref, mag, n_ops, out)
    d = np.abs(got - ref)
    viol = d > b
    ratio = np.where(b > 0, d / np.where(b > 0, b, 1.0), np.where(d > 0, np.inf, 0.0))
    info = {"ok": not bool(viol.any()), "worst": float(ratio.max()), "nviol": int(viol.sum()), "n": int(ref.size)}
    if viol.any():
        bad = np.argwhere(viol)
        ch = np.unique(bad[:, -1])
        info["first"] = [(tuple(int(v) for v in i), float(got[tuple(i)]), float(ref[tuple(i)]), float(b[tuple(i)])) for i in bad[:6]]
        info["bad_channels"] = [int(c) for c in ch[:32]]
        info["n_bad_channels"] = int(ch.size)
    return info


def rounding_bias(got, ref, out="bf16"):
    got, ref = np.asarray(got, F64), np.asarray(ref, F64)
    sel = np.abs(ref) >= 2.0 ** -6
    n = int(sel.sum())
    if n == 0:
        return 0.0, 0
    r = ref[sel]
    ulp = 2.0 * half_ulp_out(np.abs(r), out)
    return float(np.mean(np.sign(r) * (got[sel] - r) / ulp)), n


def check_bias(got, ref, out="bf16"):
    b, n = rounding_bias(got, ref, out)
    return {"ok": bool(n >= BIAS_MIN_ELEMS and abs(b) <= BIAS_LIMIT), "bias": b, "n_bias": n}


# ------------------------------------------------------------------------------------------------ numpy emulation of the kernel contract
def bf16_truncate(a):
    a = np.ascontiguousarray(np.asarray(a, np.float32))
    return (a.view(np.uint32) & np.uint32(0xffff0000)).view(np.float32)


def emulate(x, w, scale, shift, res, act, store="rne", drop_shift_channel=None, relu_skip_above=None, drop_chunk=None, chunk=16):
    """y = store_bf16(act(fp32 accumulation of x . w^T in `chunk`-wide steps, * scale + shift + res)) -- what a conv / GEMM kernel
    of this library promises.  The keyword arguments switch on ONE defect each (the mutants of test_strict_host.py):
      store="trunc"            the bf16 store truncates
      drop_shift_channel=k     channel k's BatchNorm shift is lost
      relu_skip_above=t        ReLU is skipped for pre-activations in (t, 0)
      drop_chunk=(c, n0, n1)   reduction chunk c is not accumulated for the output channels n0 .. n1 - 1"""
    x32, w32 = np.asarray(x, np.float32), np.asarray(w, np.float32)
    acc = np.zeros((x32.shape[0], w32.shape[0]), np.float32)
    for c, k0 in enumerate(range(0, x32.shape[1], chunk)):
        part = x32[:, k0:k0 + chunk] @ w32[:, k0:k0 + chunk].T
        if drop_chunk is not None and drop_chunk[0] == c:
            part[:, drop_chunk[1]:drop_chunk[2]] = 0
        acc = acc + part
    sh = np.array(shift, np.float32)
    if drop_shift_channel is not None:
        sh[drop_shift_channel] = 0
    y = acc * np.asarray(scale, np.float32) + sh
    if res is not None:
        y = y + np.asarray(res, np.float32)
    if act == 1:
        keep = (y > relu_skip_above) if relu_skip_above is not None else np.zeros(y.shape, bool)
        y = np.where((y > 0) | keep, y, np.float32(0))
    return bf16_truncate(y) if store == "trunc" else bf(y)


# ================================================================================================ memory-bound kernels
# Case data, float64 references and float32 emulations for tests/test_strict_mem_gpu.py and tests/test_strict_host.py.
F32 = np.float32
SENTINEL = -7.0               # tests/_slices.py: what a destination holds before the launch
ACT_CODES = {"none": 0, "relu": 1, "gelu_tanh": 2, "hard_swish": 3, "hard_sigmoid": 4, "sigmoid": 5, "silu": 6}
_LOG2E = F32(1.4426950408889634)
_GELU_K0 = F32(F32(-2.0) * F32(0.7978845608028654)) * _LOG2E          # common.h: folded in float by the compiler
_GELU_K1 = _GELU_K0 * F32(0.044715)


def q_of(dtype):
    """Rounds to the storage type (operands are rounded before both sides see them)."""
    return bf if dtype == "bf16" else (lambda a: np.asarray(a, F32))


def store(y, out, mode="rne"):
    """The kernel's store of an fp32 value: as it is for fp32, round-to-nearest-even for bf16 (mode="trunc": the truncating mutant)."""
    y = np.asarray(y, F32)
    if out != "bf16":
        return y
    return bf16_truncate(y) if mode == "trunc" else bf(y)


def wide_data(rng, shape, dtype):
    """Gaussian values times log-uniform magnitudes 2^-20 .. 2^20, rounded to the storage type: finite, no NaN, no subnormal."""
    g = rng.standard_normal(shape)
    g = np.where(np.abs(g) < 1e-3, 1e-3, g)
    x = q_of(dtype)(g * np.exp2(rng.uniform(-20.0, 20.0, shape)))
    assert np.isfinite(x).all() and (np.abs(x) >= 2.0 ** -40).all()
    return x


def act_input(rng, n, dtype):
    """Uniform in [-8, 8] with exact hits on -3, 0 and 3 (the corners of the hard activations)."""
    x = q_of(dtype)(rng.uniform(-8.0, 8.0, n))
    x[[0, n // 3, n - 1]] = (-3.0, 0.0, 3.0)          # the first and the last element too: the ends of the vector / scalar loop
    x[5:5 + 3 * 7:7] = (-3.0, 0.0, 3.0)
    return x


# ------------------------------------------------------------------------------------------------ activations
def act64(x, act):
    """float64 reference of common.h's apply_act_rt (jax.nn.*).  gelu_tanh: 0.5 x (1 + tanh u) = x / (1 + exp(-2 u)) -- the same
    function; the second form keeps its precision where tanh u -> -1."""
    x = np.asarray(x, F64)
    if act in (None, "none"):
        return x
    if act == "relu":
        return np.maximum(x, 0.0)
    if act == "hard_sigmoid":
        return np.clip(x + 3.0, 0.0, 6.0) / 6.0
    if act == "hard_swish":
        return x * np.clip(x + 3.0, 0.0, 6.0) / 6.0
    if act == "sigmoid":
        return 1.0 / (1.0 + np.exp(-x))
    if act == "silu":
        return x / (1.0 + np.exp(-x))
    if act == "gelu_tanh":
        u = np.sqrt(2.0 / np.pi) * (x + 0.044715 * x ** 3)
        return x / (1.0 + np.exp(-2.0 * u))
    raise ValueError(act)


def act_n_ops(x, act):
    """fp32 roundings on apply_act_rt's path (relative to |ref|, in units of 2^-23), counted from common.h:
      none / relu       0   (a select)
      hard_sigmoid      3   v + 3, the constant 1/6, the multiply (min / max are exact)
      hard_swish        4   the same and v * (.)
      sigmoid           rcp(1 + exp2(t)), t = -log2(e) v: the constant and the product round t twice; a relative error d of t is a
                        relative error |t| ln2 d <= |t| d of exp2(t), so each rounding of the argument counts |t| operations:
                        2 |t| + 2 (v_exp_f32) + 1 (the add; e / (1 + e) <= 1 passes the error of e on at most unchanged) + 2 (v_rcp_f32)
      silu              sigmoid + 1 (v * (.))
      gelu_tanh         t = x (k1 x^2 + k0): k0 and k1 are rounded constants (1 + 2: k1 = k0 * 0.044715f), x^2, the fma (both terms have
                        the same sign: no cancellation) and x * (.) make 5 roundings of t (x^2 and k1 touch one term only: counted
                        whole); 5 |t| + 2 + 1 + 2 + 1 (x * rcp)."""
    x = np.asarray(x, F64)
    if act in (None, "none", "relu"):
        return np.zeros(x.shape)
    if act == "hard_sigmoid":
        return np.full(x.shape, 3.0)
    if act == "hard_swish":
        return np.full(x.shape, 4.0)
    t = np.abs(float(_LOG2E) * x)
    if act == "sigmoid":
        return 2.0 * t + 5.0
    if act == "silu":
        return 2.0 * t + 6.0
    if act == "gelu_tanh":
        t = np.abs(x * (float(_GELU_K1) * x * x + float(_GELU_K0)))
        return 5.0 * t + 6.0
    raise ValueError(act)


def act32(v, act, relu_skip_above=None):
    """float32 emulation of apply_act_rt.  relu_skip_above=t: ReLU is skipped for pre-activations in (t, 0)."""
    v = np.asarray(v, F32)
    if act in (None, "none"):
        return v
    if act == "relu":
        keep = v > 0
        if relu_skip_above is not None:
            keep = keep | (v > F32(relu_skip_above))
        return np.where(keep, v, F32(0))
    if act in ("hard_sigmoid", "hard_swish"):
        h = np.minimum(np.maximum(v + F32(3), F32(0)), F32(6))
        return (h if act == "hard_sigmoid" else v * h) * (F32(1) / F32(6))
    with np.errstate(over="ignore"):
        if act in ("sigmoid", "silu"):
            r = F32(1) / (F32(1) + np.exp2(-_LOG2E * v).astype(F32))
            return r if act == "sigmoid" else v * r
        if act == "gelu_tanh":
            t = v * (_GELU_K1.astype(F64) * (v * v).astype(F64) + _GELU_K0.astype(F64)).astype(F32)        # fmaf
            return v * (F32(1) / (F32(1) + np.exp2(t).astype(F32)))
    raise ValueError(act)


def _drop_last_trip(y, threads):
    """The mutant `the last partial grid-stride trip is not written`: `threads` elements per trip."""
    y = np.array(y, F32)
    full = (y.size // threads) * threads
    if full < y.size:
        y.reshape(-1)[full:] = SENTINEL
    return y


def emu_eltwise(x, act, out, store_mode="rne", relu_skip_above=None, drop_last_trip=None):
    y = store(act32(x, act, relu_skip_above), out, store_mode)
    return _drop_last_trip(y, drop_last_trip) if drop_last_trip else y


def emu_add(a, b, act, out, store_mode="rne", relu_skip_above=None, drop_last_trip=None):
    y = store(act32(np.asarray(a, F32) + np.asarray(b, F32), act, relu_skip_above), out, store_mode)
    return _drop_last_trip(y, drop_last_trip) if drop_last_trip else y


def emu_cast(x, out, trunc=False):
    return store(x, out, "trunc" if trunc else "rne")


def emu_channel_scale(x, s, out, store_mode="rne"):
    """x (N, HW, C) * s (N, C)."""
    return store(np.asarray(x, F32) * np.asarray(s, F32)[:, None, :], out, store_mode)


def emu_channel_affine(x, scale, shift, res, act, out, vec8=True, store_mode="rne", shift_from=0, drop_res_last_vec=False,
                       relu_skip_above=None):
    """act(x * scale[c] + shift[c] + res) over (rows, C).  vec8: one fma then the residual add (channel_affine_vec8_kernel); else a
    multiply and an add (channel_affine_kernel).  Mutants: shift_from=8 reads the shift of channel c + 8; drop_res_last_vec loses the
    residual of the last 8-wide vector of the tensor."""
    x = np.asarray(x, F32)
    C = x.shape[-1]
    sc = np.ones(C, F32) if scale is None else np.asarray(scale, F32)
    sh = np.zeros(C, F32) if shift is None else np.asarray(shift, F32)
    if shift_from:
        sh = np.roll(sh, -shift_from)
    if vec8:
        v = (x.astype(F64) * sc.astype(F64) + sh.astype(F64)).astype(F32)
    else:
        v = x * sc + sh
    if res is not None:
        r = np.array(res, F32)
        if drop_res_last_vec:
            r[-1, -8:] = 0
        v = v + r
    return store(act32(v, act, relu_skip_above), out, store_mode)


# ------------------------------------------------------------------------------------------------ channel scale / affine data
def scale_data(C, dtype):
    """x (3, 50, C) Gaussian; scales Gaussian with negatives and, every third one, a value in (0, 2^-6)."""
    rng = rng_of(42)
    x = q_of(dtype)(rng.standard_normal((3, 50, C)))
    s = rng.standard_normal((3, C))
    s[:, ::3] = rng.uniform(2.0 ** -12, 2.0 ** -6.5, s[:, ::3].shape)
    s = q_of(dtype)(s)
    assert (s < 0).any() and ((s > 0) & (s < 2.0 ** -6)).any()
    return x, s


def affine_data(rows, C, dtype, use_scale=True, use_shift=True, res=False, seed=43):
    rng = rng_of(seed)
    q = q_of(dtype)
    x = q(rng.standard_normal((rows, C)))
    sc = gauss_scale(rng, C) if use_scale else None
    sh = rng.standard_normal(C).astype(F32) if use_shift else None
    r = q(rng.standard_normal((rows, C))) if res else None
    return x, sc, sh, r


def affine_ref(x, sc, sh, r, act):
    return epilogue64(x.astype(F64), np.abs(x).astype(F64), sc, sh, r, ACT_CODES[act])


# ------------------------------------------------------------------------------------------------ pools
def pool_out(n, k, s, p):
    return (n + 2 * p - k) // s + 1


def maxpool64(x, k, s, p):
    """x (N, H, W, C): reduce_window(max) with -inf padding."""
    y = torch.nn.functional.max_pool2d(_t(x).permute(0, 3, 1, 2), k, s, p)
    return y.permute(0, 2, 3, 1).contiguous().numpy()


def emu_maxpool(x, k, s, p, pad_value=-np.inf):
    """pad_value=0: the mutant that reads a padded tap as 0."""
    x = np.asarray(x, F32)
    N, H, W, C = x.shape
    Ho, Wo = pool_out(H, k, s, p), pool_out(W, k, s, p)
    xp = np.full((N, H + 2 * p, W + 2 * p, C), pad_value, F32)
    xp[:, p:p + H, p:p + W] = x
    y = np.full((N, Ho, Wo, C), -np.inf, F32)
    for r in range(k):
        for c in range(k):
            y = np.maximum(y, xp[:, r:r + (Ho - 1) * s + 1:s, c:c + (Wo - 1) * s + 1:s])
    return y


def adaptive_ref(x, oh, ow):
    """(ref, mag, window sizes) of the adaptive average pool of x (N, H, W, C) in float64; mag = the window's mean of |x|."""
    x = np.asarray(x, F64)
    N, H, W, C = x.shape
    hb, wb = O._adaptive_bounds(H, oh), O._adaptive_bounds(W, ow)
    ref, mag, win = np.empty((N, oh, ow, C)), np.empty((N, oh, ow, C)), np.empty((N, oh, ow, C))
    for i, (h0, h1) in enumerate(hb):
        for j, (w0, w1) in enumerate(wb):
            ref[:, i, j] = x[:, h0:h1, w0:w1].mean(axis=(1, 2))
            mag[:, i, j] = np.abs(x[:, h0:h1, w0:w1]).mean(axis=(1, 2))
            win[:, i, j] = (h1 - h0) * (w1 - w0)
    return ref, mag, win


def emu_adaptive_avgpool(x, oh, ow, out, store_mode="rne", neighbour_count=False):
    """adaptive_avgpool_nhwc_kernel: a sequential fp32 sum over the window, one division by its size.  neighbour_count: the mutant
    that divides by the size of the window to the right."""
    x = np.asarray(x, F32)
    N, H, W, C = x.shape
    hb, wb = O._adaptive_bounds(H, oh), O._adaptive_bounds(W, ow)
    y = np.empty((N, oh, ow, C), F32)
    for i, (h0, h1) in enumerate(hb):
        for j, (w0, w1) in enumerate(wb):
            s = np.zeros((N, C), F32)
            for hh in range(h0, h1):
                for ww in range(w0, w1):
                    s = s + x[:, hh, ww]
            n0, n1 = wb[(j + 1) % ow] if neighbour_count else (w0, w1)
            y[:, i, j] = s / F32((h1 - h0) * (n1 - n0))
    return store(y, out, store_mode)


def wide_geometry(C):
    """pool.hip, mv_adaptive_avgpool2d_nhwc_fwd: (cpb, pl, idle threads, channel blocks) of global_avgpool_wide_kernel."""
    c8 = C // 8
    cpb = min(c8, 32)
    pl = 1024 // cpb
    return cpb, pl, 1024 - cpb * pl, -(-c8 // cpb)


def emu_global_avgpool(x, out, pl=1, store_mode="rne", lost_lane=None):
    """x (N, HW, C).  Lane lp of `pl` adds the pixels lp, lp + pl, ... in order; lane 0 then adds the other lanes' sums in order and
    multiplies by 1 / HW (global_avgpool_wide_kernel; pl = 1 is global_avgpool_bf16x8_kernel).  lost_lane=q: lane q's sum is lost."""
    x = np.asarray(x, F32)
    N, HW, C = x.shape
    part = np.zeros((N, pl, C), F32)
    for p0 in range(0, HW, pl):
        chunk = x[:, p0:p0 + pl]
        part[:, :chunk.shape[1]] = part[:, :chunk.shape[1]] + chunk
    s = part[:, 0]
    for q in range(1, pl):
        if q != lost_lane:
            s = s + part[:, q]
    return store(s * (F32(1) / F32(HW)), out, store_mode)


def avgpool2d_ref(x, k, s):
    x = np.asarray(x, F64)
    N, H, W, C = x.shape
    Ho, Wo = pool_out(H, k, s, 0), pool_out(W, k, s, 0)
    ref, mag = np.zeros((N, Ho, Wo, C)), np.zeros((N, Ho, Wo, C))
    for r in range(k):
        for c in range(k):
            v = x[:, r:r + (Ho - 1) * s + 1:s, c:c + (Wo - 1) * s + 1:s]
            ref, mag = ref + v, mag + np.abs(v)
    return ref / (k * k), mag / (k * k)


def emu_avgpool2d(x, k, s, out, store_mode="rne"):
    """avgpool2d_nhwc_kernel: fp32 sum in (dy, dx) order, times 1 / (k k)."""
    x = np.asarray(x, F32)
    N, H, W, C = x.shape
    Ho, Wo = pool_out(H, k, s, 0), pool_out(W, k, s, 0)
    a = np.zeros((N, Ho, Wo, C), F32)
    for r in range(k):
        for c in range(k):
            a = a + x[:, r:r + (Ho - 1) * s + 1:s, c:c + (Wo - 1) * s + 1:s]
    return store(a * (F32(1) / F32(k * k)), out, store_mode)


# ------------------------------------------------------------------------------------------------ bilinear resize
def taps32(n_in, n_out, clamp=True):
    """resize.hip's taps_for in float32: (i0, i1, w1) per output index.  clamp=False: the mutant that leaves i1 = n_in at the last
    half pixel."""
    o = np.arange(n_out, dtype=F32)
    src = (o + F32(0.5)) * (F32(n_in) / F32(n_out)) - F32(0.5)
    f = np.floor(src)
    i0, w1 = f.astype(np.int64), (src - f).astype(F32)
    i1 = i0 + 1
    i0 = np.maximum(i0, 0)
    if clamp:
        i1 = np.minimum(i1, n_in - 1)
    return i0, i1, w1


def tap_matrix32(n_in, n_out):
    """The (n_in, n_out) weight matrix that taps32 stands for, in float64 arithmetic on the float32 weights."""
    i0, i1, w1 = taps32(n_in, n_out)
    m = np.zeros((n_in, n_out))
    np.add.at(m, (i0, np.arange(n_out)), 1.0 - w1.astype(F64))
    np.add.at(m, (i1, np.arange(n_out)), w1.astype(F64))
    return m


def resize_ref(x, H, W):
    """jax.image.resize(bilinear) of x (N, h, w, C) in float64 (oracle weights); also M = max |x| per image and channel."""
    x = np.asarray(x, F64)
    ref = np.einsum("nhwc,hH,wW->nHWc", x, O._resize_weights(x.shape[1], H), O._resize_weights(x.shape[2], W))
    M = np.broadcast_to(np.abs(x).max(axis=(1, 2))[:, None, None, :], ref.shape)
    return ref, M


def resize_bound(ref, M, h, w, out):
    """(8 + 2 max(h, w)) 2^-23 M + half_ulp_out: 8 for the six fp32 operations of the two-level interpolation (each on values <= 2 M);
    a source coordinate below max(h, w) carries an fp32 rounding of that size, i.e. 2 max(h, w) 2^-23 M through (v1 - v0) w1."""
    e = (8 + 2 * max(h, w)) * 2.0 ** -23 * np.asarray(M, F64)
    return e + half_ulp_out(np.abs(ref) + e, out)


def emu_resize(x, H, W, out, nchw=False, store_mode="rne", clamp=True):
    """resize_bilinear_kernel in float32: top = v00 + (v01 - v00) wx, bot likewise, top + (bot - top) wy.  clamp=False: the
    unclamped tap reads the next pixel in memory (the first pixel of the next row; emulated as a wrap)."""
    x = np.asarray(x, F32)
    N, h, w, C = x.shape
    y0, y1, wy = taps32(h, H, clamp)
    x0, x1, wx = taps32(w, W, clamp)
    rows0, rows1 = np.take(x, y0, 1, mode="wrap"), np.take(x, y1, 1, mode="wrap")
    v00, v01 = np.take(rows0, x0, 2, mode="wrap"), np.take(rows0, x1, 2, mode="wrap")
    v10, v11 = np.take(rows1, x0, 2, mode="wrap"), np.take(rows1, x1, 2, mode="wrap")
    wxb, wyb = wx[None, None, :, None], wy[None, :, None, None]
    top = v00 + (v01 - v00) * wxb
    bot = v10 + (v11 - v10) * wxb
    y = top + (bot - top) * wyb
    if nchw:
        y = np.ascontiguousarray(y.transpose(0, 3, 1, 2))
    return store(y, out, store_mode)


# ------------------------------------------------------------------------------------------------ backward kernels (fp32)
def emu_channel_scale_bwd(g, x):
    """channel_scale_bwd_kernel: four row groups (p = rg, rg + 4, ...) of fma, then (p0 + p1) + (p2 + p3).  g, x (B, HW, C)."""
    g, x = np.asarray(g, F32), np.asarray(x, F32)
    part = []
    for rg in range(4):
        acc = np.zeros((g.shape[0], g.shape[2]), F32)
        for p in range(rg, g.shape[1], 4):
            acc = (g[:, p].astype(F64) * x[:, p].astype(F64) + acc.astype(F64)).astype(F32)
        part.append(acc)
    return (part[0] + part[1]) + (part[2] + part[3])


def bn_dz_coef64(s1, s2, s0, mean, var, scale, n, a, eps):
    """include/eqxvision_amd.h, mv_bn_train_dz_coef_f32: B = -(a / n) scale rstd^2 (sum dy z - mean sum dy),
    A = -(a / n) scale sum dy - B sum_z / n; with the magnitudes of the bound (the error of B goes into A's):
      B: a / n (2), var + eps, 1 / (.) (2), two products, mean * s1, the difference, the last product: 10 roundings of
         magB = |k scale r2| (|s2| + |mean s1|);
      A: k (2), two products | s0 / n (2), the product | the difference: 5 roundings of |k scale s1| + |B s0 / n|, and B's own error
         (<= 11 2^-23 magB with its store) times |s0 / n|: 16 roundings of magA = |k scale s1| + (|B| + magB) |s0 / n|."""
    s1, s2, s0, mean, var, scale = (np.asarray(v, F64) for v in (s1, s2, s0, mean, var, scale))
    k = float(a) / float(n)
    r2 = 1.0 / (var + float(eps))
    B = -k * scale * r2 * (s2 - mean * s1)
    magB = np.abs(k * scale * r2) * (np.abs(s2) + np.abs(mean * s1))
    A = -k * scale * s1 - B * (s0 / n)
    magA = np.abs(k * scale * s1) + (np.abs(B) + magB) * np.abs(s0 / n)
    return A, magA, B, magB
