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

The last part does the same for the training backward kernels (csrc/train_bwd.hip; tests/test_strict_bwd_gpu.py, proofs in
tests/test_strict_bwd_host.py): the conv shapes, float64 autograd references, and emulations of the input- and weight-gradient
contracts, the column sum and the attention backward, again one defect switch each.
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


def epilogue64(acc, amag, scale, shift, res, act, pre=False):
    """(ref, mag) of act(acc * scale + shift + res) with the channel last; `amag` is the contraction of the absolute values and `mag`
    the magnitude of the PRE-activation.  `act` is an MV_ACT_* code or name; pre=True adds the float64 pre-activation, which the
    bound of an activation beyond none / ReLU is computed from (act_bound)."""
    p, mag = acc, amag
    if scale is not None:
        p = p * np.asarray(scale, F64)
        mag = mag * np.abs(np.asarray(scale, F64))
    if shift is not None:
        p = p + np.asarray(shift, F64)
        mag = mag + np.abs(np.asarray(shift, F64))
    if res is not None:
        p = p + np.asarray(res, F64)
        mag = mag + np.abs(np.asarray(res, F64))
    ref = act64(p, act_name(act))
    return (ref, mag, p) if pre else (ref, mag)


def conv_ref(x_nhwc, w_krsc, scale, shift, res, act, stride=1, pad=0, dil=1, groups=1, pre=False):
    acc = _conv64(x_nhwc, w_krsc, stride, pad, dil, groups)
    amag = _conv64(np.abs(x_nhwc), np.abs(w_krsc), stride, pad, dil, groups)
    return epilogue64(acc, amag, scale, shift, res, act, pre)


def gemm_ref(x, w, scale, shift, res, act, pre=False):
    x, w = np.asarray(x, F64), np.asarray(w, F64)
    return epilogue64(x @ w.T, np.abs(x) @ np.abs(w).T, scale, shift, res, act, pre)


# ------------------------------------------------------------------------------------------------ instrument 1
def prove_exact(name, ref, mag, weights, stored=(), hidden=(), out="bf16", min_nonzero=0.10, frac_bits=0, hidden_max=BF16_INT_MAX):
    """The exact-integer preconditions, asserted on the CPU before a launch (the float64 arrays hold integers far below 2^53, so the
    conversion to int64 is itself exact and checked):
      (a) `mag` (sum |x||w| * |scale| + |shift| + |res|) <= 256 for a bf16 output, and every operand in `stored` / intermediate in
          `hidden` is an integer of magnitude <= 256; mag < 2^24 for the fp32 accumulators;
      (b) every reduction index of every matrix in `weights` ((rows, reduction) layout) has a non-zero weight in some row, and every
          row has a non-zero weight;
      (c) fewer than 90 % of the reference outputs are zero.
    `frac_bits` = f: "integer" reads "multiple of 2^-f" and the limits apply to the value times 2^f (dyadic operands: an average over
    4 or 16 pixels, bilinear taps at ratio 2); `hidden_max` replaces the bf16 limit of `stored` / `hidden` where nothing is stored
    as bf16 (the fp32 gradient path: tests/_rule_grad.py)."""
    for what, a in [("ref", ref), ("mag", mag)] + [(f"stored[{i}]", s) for i, s in enumerate(stored)] + \
                   [(f"hidden[{i}]", h) for i, h in enumerate(hidden)]:
        a = np.ldexp(np.asarray(a, F64), frac_bits)
        ai = np.rint(a).astype(np.int64)
        assert np.array_equal(ai.astype(F64), a), f"{name}: {what} is not integer-valued"
        top = int(np.abs(ai).max()) if ai.size else 0
        assert top < ACC_INT_MAX, f"{name}: {what} reaches {top} >= 2^24 (fp32 accumulator not exact)"
        if out == "bf16" or what not in ("ref", "mag"):
            lim = BF16_INT_MAX if what in ("ref", "mag") else hidden_max
            assert top <= lim, f"{name}: {what} reaches {top} > {lim} (not exact in bf16)"
    _prove_coverage(name, weights)
    zeros = float((np.asarray(ref) == 0).mean())
    assert zeros < 1.0 - min_nonzero, f"{name}: {100 * zeros:.1f} % of the reference outputs are zero (ReLU blanks the test)"


def _prove_coverage(name, weights):
    for i, w in enumerate(weights):
        w2 = np.asarray(w).reshape(w.shape[0], -1) != 0
        assert w2.any(axis=0).all(), f"{name}: weights[{i}] leaves {int((~w2.any(axis=0)).sum())} reduction indices unused"
        assert w2.any(axis=1).all(), f"{name}: weights[{i}] has {int((~w2.any(axis=1)).sum())} all-zero output channels"


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


ACT_DEFECTS = ("skip_tail_vec", "act_before_res", "act_before_shift", "trunc", "erf_gelu", "pair_repeat", "no_clamp6")


def emulate(x, w, scale, shift, res, act, store="rne", drop_shift_channel=None, relu_skip_above=None, drop_chunk=None, chunk=16,
            out="bf16", skip_tail_vec=False, act_before_res=False, act_before_shift=False, erf_gelu=False, pair_repeat=False,
            no_clamp6=False):
    """y = store_out(act(fp32 accumulation of x . w^T in `chunk`-wide steps, * scale + shift + res)) -- what a conv / GEMM kernel
    of this library promises; `act` is an MV_ACT_* code or name (act32).  The keyword arguments switch on ONE defect each (the
    mutants of test_strict_host.py and test_strict_act_host.py):
      store="trunc"            the bf16 store truncates (after the activation)
      drop_shift_channel=k     channel k's BatchNorm shift is lost
      relu_skip_above=t        ReLU is skipped for pre-activations in (t, 0)
      drop_chunk=(c, n0, n1)   reduction chunk c is not accumulated for the output channels n0 .. n1 - 1
      skip_tail_vec            the activation is skipped on the last 8-wide vector of the output channels (a ragged tile's tail)
      act_before_res           the activation is applied before the residual add
      act_before_shift         the activation is applied before the shift (and the residual)
      erf_gelu                 0.5 v (1 + erf(v / sqrt 2)) instead of the tanh form
      pair_repeat              the second value of every packed pair repeats the first (gelu_tanh_pack2's lanes)
      no_clamp6                hard-swish without the clamp at 6: v max(v + 3, 0) / 6"""
    name = act_name(act)

    def activate(v):
        if erf_gelu and name == "gelu_tanh":
            t = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32))
            return (np.float32(0.5) * t * (1 + torch.erf(t * np.float32(0.7071067811865476)))).numpy()
        if no_clamp6 and name == "hard_swish":
            return v * np.maximum(v + np.float32(3), np.float32(0)) * (np.float32(1) / np.float32(6))
        return act32(v, name, relu_skip_above)
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
    v = acc if scale is None else acc * np.asarray(scale, np.float32)
    r = np.float32(0) if res is None else np.asarray(res, np.float32)
    if act_before_shift:
        y = (activate(v) + sh) + r
    elif act_before_res:
        y = activate(v + sh) + r
    else:
        y = activate((v + sh) + r)
    if skip_tail_vec:
        y = np.array(y, np.float32)
        y[:, -8:] = ((v + sh) + r)[:, -8:]
    if pair_repeat:
        y = np.array(y, np.float32)
        y[:, 1::2] = y[:, 0:y.shape[1] - y.shape[1] % 2:2]
    if out != "bf16":
        return np.asarray(y, np.float32)
    return bf16_truncate(y) if store == "trunc" else bf(y)


# ================================================================================================ memory-bound kernels
# Case data, float64 references and float32 emulations for tests/test_strict_mem_gpu.py and tests/test_strict_host.py.
F32 = np.float32
SENTINEL = -7.0               # tests/_slices.py: what a destination holds before the launch
ACT_CODES = {"none": 0, "relu": 1, "gelu_tanh": 2, "hard_swish": 3, "hard_sigmoid": 4, "sigmoid": 5, "silu": 6}
ACT_NAMES = {v: k for k, v in ACT_CODES.items()}


def act_name(act):
    """An MV_ACT_* code, a name or None -> the name."""
    return "none" if act is None else (ACT_NAMES[int(act)] if not isinstance(act, str) else act)


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
    with np.errstate(over="ignore"):                     # exp -> inf gives the limit 0 / -0
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


# ================================================================================================ training backward kernels
# Case data, float64 references and float32 emulations for tests/test_strict_bwd_gpu.py and tests/test_strict_bwd_host.py
# (csrc/train_bwd.hip; every kernel there is fp32).
def int_nz(rng, shape, lim):
    """Integers in [-lim, lim] without 0, as float32 (a depthwise filter has one channel: a zero tap would be an unused index)."""
    return (rng.integers(1, lim + 1, shape) * rng.choice(np.array([-1, 1]), shape)).astype(F32)


def eighths(rng, shape):
    """Multiples of 1/8 in [0, 1]: stand-ins for probabilities whose products with small integers are exact in fp32."""
    return (rng.integers(0, 9, shape) / 8.0).astype(F32)


def _pair(v):
    return (int(v[0]), int(v[1])) if isinstance(v, (tuple, list)) else (int(v), int(v))


class ConvGeom:
    """One conv shape (N, H, W, C, K, (R, S), stride, pad, dil, groups); stride / pad / dil one int or an (h, w) pair."""

    def __init__(self, N, H, W, C, K, RS, stride, pad, dil, groups):
        self.N, self.H, self.W, self.C, self.K, self.groups = N, H, W, C, K, groups
        (self.R, self.S), (self.sh, self.sw), (self.ph, self.pw), (self.dh, self.dw) = _pair(RS), _pair(stride), _pair(pad), _pair(dil)
        self.Ho = (H + 2 * self.ph - self.dh * (self.R - 1) - 1) // self.sh + 1
        self.Wo = (W + 2 * self.pw - self.dw * (self.S - 1) - 1) // self.sw + 1
        self.Cg, self.Kg, self.P = C // groups, K // groups, N * self.Ho * self.Wo
        self.out_elems = K * self.R * self.S * self.Cg
        self.tag = f"{N}x{H}x{W}_C{C}_K{K}_{self.R}x{self.S}_s{self.sh}{self.sw}_p{self.ph}{self.pw}_d{self.dh}{self.dw}_g{groups}"

    def args(self):
        """The entries' argument tail: N, H, W, C, K, R, S, sh, sw, ph, pw, dh, dw, groups."""
        return (self.N, self.H, self.W, self.C, self.K, self.R, self.S, self.sh, self.sw, self.ph, self.pw, self.dh, self.dw, self.groups)

    def wgrad_split(self, offer_bytes=None):
        """mv_conv2d_wgrad_nhwc_f32's arithmetic as its comment states it: tiles x position chunks ~ 4096 waves, at least 128
        positions per chunk, at most 1024 chunks; (split the entry wants, split it runs with an offer of `offer_bytes`)."""
        tiles = self.groups * -(-self.Kg // 32) * -(-self.Cg // 32) * self.R * self.S
        want = 1 if tiles >= 2048 else -(-4096 // tiles)
        want = min(want, (self.P + 127) // 128, 1024)
        if want <= 1:
            return want, 1
        have = max((offer_bytes or 0) - 4096, 0)
        fit = have // (self.out_elems * 4)
        return want, (1 if fit < 2 else min(want, fit))


# the issue's ten shapes; the eleventh is the one whose own split exceeds 2 (P = 396: four chunks), which none of the ten reaches
CONV_BWD_SHAPES = [ConvGeom(*s) for s in [
    (1, 9, 11, 40, 21, (1, 1), 1, 0, 1, 1),           # scalar-k loop, odd K, ragged second channel tile, M = 99 < 128
    (2, 7, 9, 24, 12, (3, 3), 2, 1, 1, 1),            # float4 loop with K % 8 == 4 (P = 2 * 4 * 5 is even: odd P comes from 99 and 9)
    (1, 8, 8, 16, 6, (3, 3), 1, 2, 2, 1),             # K % 4 == 2, dilation
    (1, 9, 12, 8, 8, (1, 7), (2, 1), (0, 3), 1, 1),   # R != S, sh != sw, ph != pw; C = 8: the MFMA gate's edge
    (1, 9, 12, 7, 8, (1, 7), (2, 1), (0, 3), 1, 1),   # C = 7: the VALU kernel serves it
    (3, 5, 3, 16, 40, (3, 3), 1, 0, 1, 1),            # Wo = 1 (P = 9, odd), two k tiles, the second ragged
    (2, 6, 4, 16, 8, (3, 3), 1, 0, 1, 1),             # Wo = 2
    (2, 7, 7, 12, 12, (3, 3), 2, 1, 1, 12),           # depthwise
    (2, 6, 6, 12, 20, (3, 3), 1, 1, 1, 4),            # Kg = 5, Cg = 3
    (1, 12, 11, 72, 8, (3, 3), 1, 1, 1, 1),           # M = 132: two blocks, three channel tiles; split = 2
    (3, 12, 11, 40, 21, (3, 3), 1, 1, 1, 1),          # P = 396: the entry wants split = 4 (the clamp cases)
]]
CONV_BWD_CLAMP = CONV_BWD_SHAPES[-1]


def conv_bwd_data(g, kind, seed=60):
    """(x NHWC, w KRSC, dy NHWK) float32: kind "int" -> integers in [-2, 2] (w and dy without zeros), "gauss" -> Gaussian, the
    filter scaled by 1 / sqrt(fan-in)."""
    rng = rng_of(seed + (0 if kind == "int" else 1))
    xs, ws, ys = (g.N, g.H, g.W, g.C), (g.K, g.R, g.S, g.Cg), (g.N, g.Ho, g.Wo, g.K)
    if kind == "int":
        return int_tensor(rng, xs, 2), int_nz(rng, ws, 2), int_nz(rng, ys, 2)
    return (rng.standard_normal(xs).astype(F32), (rng.standard_normal(ws) / np.sqrt(g.Cg * g.R * g.S)).astype(F32),
            rng.standard_normal(ys).astype(F32))


def conv_bwd64(x_nhwc, w_krsc, dy_nhwk, g):
    """(dx NHWC, dw KRSC) of sum(conv2d(x, w) * dy): float64 torch.autograd of F.conv2d on double tensors."""
    x = _t(x_nhwc).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    w = _t(w_krsc).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    y = torch.nn.functional.conv2d(x, w, None, (g.sh, g.sw), (g.ph, g.pw), (g.dh, g.dw), g.groups)
    gx, gw = torch.autograd.grad(y, (x, w), _t(dy_nhwk).permute(0, 3, 1, 2).contiguous())
    return gx.permute(0, 2, 3, 1).contiguous().numpy(), gw.permute(0, 2, 3, 1).contiguous().numpy()


def conv_bwd_ref(x, w, dy, g):
    """(dx, mag of dx, dw, mag of dw): the references and the same contractions on absolute values."""
    dx, dw = conv_bwd64(x, w, dy, g)
    mx, mw = conv_bwd64(np.abs(x), np.abs(w), np.abs(dy), g)
    return dx, mx, dw, mw


def conv_bwd_weights(x, w, dy, g):
    """The (rows, reduction) matrices prove_exact looks at: per group the filters as (channel, (k, r, s)) for the input gradient;
    dy as (k, position) and x as (channel, pixel) for the weight gradient."""
    per_group = [w[i * g.Kg:(i + 1) * g.Kg].transpose(3, 0, 1, 2).reshape(g.Cg, -1) for i in range(g.groups)]
    return per_group, [dy.reshape(-1, g.K).T, x.reshape(-1, g.C).T]


def _mm32(a, b):
    return np.asarray(a, F32) @ np.asarray(b, F32)


def emu_conv_dgrad(dy, w, g, defect=None):
    """The input-gradient contract in float32: dx[pos][c] = sum over the taps (r, s) whose stride divides of dy[out(pos, r, s)] . w[:, r, s, c]
    (conv_dgrad_mfma_kernel; one fp32 matrix product per tap).  Defects, one each:
      "drop_last_odd_k"   the scalar-k loop's last step is lost when K is odd (k = K - 1 sits alone in its pair)
      "read_past_k"       the float4 loop keeps the upper half-wave's four k when K % 8 == 4: it reads dy[pos][K .. K + 3] -- the next
                          position's first four values, the sentinel behind the last -- against four filters past the end (sentinel)
      "stride_any"        a tap is accepted where the stride does not divide (ho = th / sh without the remainder test)"""
    dy, w = np.asarray(dy, F32), np.asarray(w, F32)
    K = g.K
    dyf = dy.reshape(-1, K)
    if defect == "drop_last_odd_k" and K % 2:
        dyf = dyf.copy()
        dyf[:, K - 1] = 0
    if defect == "read_past_k" and K % 8 == 4:
        assert g.groups == 1
        flat = np.concatenate([dyf.reshape(-1), np.full(4, SENTINEL, F32)])
        idx = np.arange(dyf.shape[0])[:, None] * K + np.arange(K + 4)[None, :]
        dyf = flat[idx]
        w = np.concatenate([w, np.full((4,) + w.shape[1:], SENTINEL, F32)])
        K = K + 4
    Kg = K // g.groups
    dx = np.zeros((g.N * g.H * g.W, g.C), F32)
    m = np.arange(g.N * g.H * g.W)
    wi, hi, n = m % g.W, (m // g.W) % g.H, m // (g.W * g.H)
    for r in range(g.R):
        th = hi + g.ph - r * g.dh
        ho = np.floor_divide(th, g.sh)
        hok = (th >= 0) & (ho < g.Ho) & ((th % g.sh == 0) | (defect == "stride_any"))
        for s in range(g.S):
            tw = wi + g.pw - s * g.dw
            wo = np.floor_divide(tw, g.sw)
            ok = hok & (tw >= 0) & (wo < g.Wo) & ((tw % g.sw == 0) | (defect == "stride_any"))
            rows = dyf[np.where(ok, (n * g.Ho + ho) * g.Wo + wo, 0)] * ok[:, None].astype(F32)
            for gi in range(g.groups):
                dx[:, gi * g.Cg:(gi + 1) * g.Cg] += _mm32(rows[:, gi * Kg:(gi + 1) * Kg], w[gi * Kg:(gi + 1) * Kg, r, s, :])
    return dx.reshape(g.N, g.H, g.W, g.C)


def emu_conv_wgrad(x, dy, g, split=1, defect=None):
    """The weight-gradient contract in float32 (conv_wgrad_mfma_kernel + sum_parts_kernel): the positions p = (n, ho, wo) are cut
    into `split` chunks of an even length; each half-wave walks its chunk two positions at a time, carrying (n, ho, wo) along; the
    chunks' partial filters are added in chunk order.  Defects, one each:
      "drop_last_odd_p"   the last position of an odd P (the lower half-wave alone in its pair) is lost
      "wrap_once"         the walk's `while (wo >= Wo)` is an `if`: at Wo = 1 a step of two wraps once only and wo stays out of range
      "chunk_twice"       a chunk also takes the first position of the next one"""
    x, dy = np.asarray(x, F32), np.asarray(dy, F32)
    P = g.P
    chunk = (-(-P // split) + 1) & ~1
    dyf = dy.reshape(P, g.K)
    total = np.zeros((g.K, g.R, g.S, g.Cg), F32)
    for ci in range(split):
        p0, p1 = ci * chunk, min(ci * chunk + chunk, P)
        ps, ns, hos, wos = [], [], [], []
        for fh in (0, 1):
            p = p0 + fh
            n, rem = divmod(p, g.Ho * g.Wo)
            ho, wo = divmod(rem, g.Wo)
            last = p1 + (1 if defect == "chunk_twice" and p1 < P else 0)
            while p - fh < last:
                if p < last and not (defect == "drop_last_odd_p" and P % 2 and p == P - 1):
                    ps.append(p), ns.append(n), hos.append(ho), wos.append(wo)
                p += 2
                wo += 2
                while wo >= g.Wo:
                    wo -= g.Wo
                    ho += 1
                    if ho >= g.Ho:
                        ho, n = 0, n + 1
                    if defect == "wrap_once":
                        break
        part = np.zeros_like(total)
        if ps:
            ps, ns, hos, wos = (np.asarray(v) for v in (ps, ns, hos, wos))
            for r in range(g.R):
                hi = hos * g.sh - g.ph + r * g.dh
                for s in range(g.S):
                    wi = wos * g.sw - g.pw + s * g.dw
                    ok = (hi >= 0) & (hi < g.H) & (wi >= 0) & (wi < g.W) & (ns < g.N)
                    xr = x[np.where(ok, ns, 0), np.where(ok, hi, 0), np.where(ok, wi, 0)] * ok[:, None].astype(F32)
                    for gi in range(g.groups):
                        part[gi * g.Kg:(gi + 1) * g.Kg, r, s, :] = _mm32(dyf[ps][:, gi * g.Kg:(gi + 1) * g.Kg].T, xr[:, gi * g.Cg:(gi + 1) * g.Cg])
        total = total + part
    return total


def colsum_ref(a, b):
    a = np.asarray(a, F64)
    bb = 1.0 if b is None else np.asarray(b, F64)
    return (a * bb).sum(0), (np.abs(a) * np.abs(bb)).sum(0)


def colsum_split(M):
    """mv_colsum_f32's arithmetic: (parts, rows per part) with scratch on offer; one part below 512 rows."""
    split = min((M + 255) // 256, 512) if M >= 512 else 1
    return split, -(-M // split)


def colsum_n_ops(M, split):
    """Roundings on the longest path of one column sum, counted from colsum_kernel / colsum_part_kernel / sum_parts_kernel: the
    product, ceil(rows / 4) adds in a row group, two adds across the four groups, and `split` adds over the parts."""
    rows = -(-M // split)
    return 1 + -(-rows // 4) + 2 + (split if split > 1 else 0)


def emu_colsum(a, b=None, split=1, drop_tail_rows=False):
    """colsum_kernel (split = 1) / colsum_part_kernel + sum_parts_kernel in float32: four row groups (m = rg, rg + 4, ...) summed in
    order, (g0 + g1) + (g2 + g3), the parts added in order.  drop_tail_rows: the rows m >= 4 (M / 4) of a part are lost (a loop over
    whole groups of four)."""
    a = np.asarray(a, F32)
    v = a if b is None else a * np.asarray(b, F32)
    M, C = v.shape
    chunk = -(-M // split)
    out = np.zeros(C, F32)
    for ci in range(split):
        blk = v[ci * chunk:min((ci + 1) * chunk, M)]
        n4 = blk.shape[0] // 4
        acc = np.zeros((4, C), F32)
        for i in range(n4):
            acc += blk[4 * i:4 * i + 4]
        tail = blk[4 * n4:]
        if tail.shape[0] and not drop_tail_rows:
            acc[:tail.shape[0]] += tail
        part = (acc[0] + acc[1]) + (acc[2] + acc[3])
        out = part if split == 1 else out + part
    return out


def softmax_bwd_ref(p, dp, scale):
    """ds = scale p (dp - sum_j dp p) in float64 and its magnitude |scale p| (|dp| + sum_j |dp p|)."""
    p, dp = np.asarray(p, F64), np.asarray(dp, F64)
    ref = scale * p * (dp - (p * dp).sum(-1, keepdims=True))
    mag = np.abs(scale * p) * (np.abs(dp) + np.abs(p * dp).sum(-1, keepdims=True))
    return ref, mag


def mha_bwd_data(B, N, H, dh, kind, seed=70):
    """(qkv [B, N, 3 D], probs [B, H, N, N], dout [B, N, D]) float32.  "int": integers in [-2, 2] and probabilities that are
    multiples of 1/8, independent of qkv (the kernel reads them from a buffer); "gauss": Gaussian, rows of probs a float32 softmax."""
    rng = rng_of(seed + N + (0 if kind == "int" else 1))
    D = H * dh
    if kind == "int":
        return int_tensor(rng, (B, N, 3 * D), 2), eighths(rng, (B, H, N, N)), int_tensor(rng, (B, N, D), 2)
    s = rng.standard_normal((B, H, N, N))
    e = np.exp(s - s.max(-1, keepdims=True))
    return rng.standard_normal((B, N, 3 * D)).astype(F32), (e / e.sum(-1, keepdims=True)).astype(F32), rng.standard_normal((B, N, D)).astype(F32)


def _heads(a, H, dh):
    """[B, N, H dh] -> [B, H, N, dh]"""
    return a.reshape(a.shape[0], a.shape[1], H, dh).transpose(0, 2, 1, 3)


def mha_bwd_ref(qkv, probs, dout, scale, H, dh):
    """The four float64 contractions of train_bwd.hip's attention-backward comment: dP = dO V^T, dS = scale P (dP - sum_j P dP),
    dQ = dS K, dK = dS^T Q, dV = P^T dO; with them the magnitudes (the contractions on absolute values, dS's own magnitude carried
    through) and the operation counts of S.ops_bound, counted from mha_bwd_q_kernel / mha_bwd_kv_kernel:
      dP      dh fma
      t       its lane's ceil(N / 64) fma and 6 shuffle adds, on top of dP's
      dS      the difference and two products on top: n_ds = dh + ceil(N / 64) + 9
      dQ, dK  N fma on the stored dS: n_ds + N;   dV  N fma.
    Returns {"ds": (ref, mag, n_ops), "dqkv": (ref, mag, n_ops)}."""
    qkv, P, dout = np.asarray(qkv, F64), np.asarray(probs, F64), np.asarray(dout, F64)
    B, N, D3 = qkv.shape
    D = D3 // 3
    q, k, v = (_heads(qkv[:, :, i * D:(i + 1) * D], H, dh) for i in range(3))
    go = _heads(dout, H, dh)
    dP = go @ v.transpose(0, 1, 3, 2)
    mdP = np.abs(go) @ np.abs(v).transpose(0, 1, 3, 2)
    t = (P * dP).sum(-1, keepdims=True)
    mt = (P * mdP).sum(-1, keepdims=True)
    dS = scale * P * (dP - t)
    mdS = np.abs(scale * P) * (mdP + mt)
    n_ds = dh + -(-N // 64) + 9
    outs = [(dS @ k, mdS @ np.abs(k), n_ds + N), (dS.transpose(0, 1, 3, 2) @ q, mdS.transpose(0, 1, 3, 2) @ np.abs(q), n_ds + N),
            (P.transpose(0, 1, 3, 2) @ go, P.transpose(0, 1, 3, 2) @ np.abs(go), N)]

    def rows(a):
        return a.transpose(0, 2, 1, 3).reshape(B, N, D)
    ref = np.concatenate([rows(o[0]) for o in outs], -1)
    mag = np.concatenate([rows(o[1]) for o in outs], -1)
    n_ops = np.concatenate([np.full((B, N, D), float(o[2])) for o in outs], -1)
    return {"ds": (dS, mdS, float(n_ds)), "dqkv": (ref, mag, n_ops)}


def emu_mha_bwd(qkv, probs, dout, scale, H, dh, drop_j_tail=False):
    """mha_bwd_q_kernel + mha_bwd_kv_kernel in float32 -> (ds, dqkv).  drop_j_tail: the lane loops `for (j = lane; j < N; j += 64)`
    make one trip only: the keys j >= 64 miss from the row sum, their dS is never written (the sentinel stays) and dQ does not see
    them."""
    qkv, P, dout = np.asarray(qkv, F32), np.asarray(probs, F32), np.asarray(dout, F32)
    B, N, D3 = qkv.shape
    D = D3 // 3
    q, k, v = (_heads(qkv[:, :, i * D:(i + 1) * D], H, dh) for i in range(3))
    go = _heads(dout, H, dh)
    J = min(N, 64) if drop_j_tail else N
    dP = go @ v.transpose(0, 1, 3, 2)
    t = (P[..., :J] * dP[..., :J]).sum(-1, keepdims=True, dtype=F32)
    ds = np.full(P.shape, SENTINEL, F32)
    ds[..., :J] = F32(scale) * P[..., :J] * (dP[..., :J] - t)
    dq = ds[..., :J] @ k[:, :, :J]
    dk = ds.transpose(0, 1, 3, 2) @ q
    dv = P.transpose(0, 1, 3, 2) @ go

    def rows(a):
        return a.transpose(0, 2, 1, 3).reshape(B, N, D)
    return ds, np.concatenate([rows(dq), rows(dk), rows(dv)], -1).astype(F32)


def maxpool_bwd64(x, dy, k, s, p):
    """float64 autograd of max_pool2d: dx NHWC for x NHWC, dy NHWC (no ties in x: the gradient is defined)."""
    xt = _t(x).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    y = torch.nn.functional.max_pool2d(xt, k, s, p)
    (gx,) = torch.autograd.grad(y, (xt,), _t(dy).permute(0, 3, 1, 2).contiguous())
    return gx.permute(0, 2, 3, 1).contiguous().numpy()


def distinct_ints(rng, shape):
    """x (N, H, W, C): per channel a random permutation of 0 .. N H W - 1, centred: no two values of a channel are equal."""
    N, H, W, C = shape
    n = N * H * W
    x = np.stack([rng.permutation(n) for _ in range(C)], -1).astype(F32) - F32(n // 2)
    return x.reshape(N, H, W, C)


def patch_merge_bwd_ref(dy, H, W):
    """The adjoint of mv_patch_merge_gather_nhwc, whose blocks are (0::2, 0::2) | (1::2, 0::2) | (0::2, 1::2) | (1::2, 1::2) of the
    map padded with zeros to even sizes: dx[b, hi, wi, c] = dy[b, hi / 2, wi / 2, ((hi & 1) + 2 (wi & 1)) C + c]; what dy holds for
    the padded taps reaches no input element."""
    dy = np.asarray(dy, F64)
    B, Ho, Wo, C4 = dy.shape
    C = C4 // 4
    full = np.zeros((B, 2 * Ho, 2 * Wo, C))
    full[:, 0::2, 0::2], full[:, 1::2, 0::2] = dy[..., 0:C], dy[..., C:2 * C]
    full[:, 0::2, 1::2], full[:, 1::2, 1::2] = dy[..., 2 * C:3 * C], dy[..., 3 * C:]
    return full[:, :H, :W]


def act_grad64(x, act):
    """d act64 / dx in float64.  At the corners of the piecewise functions the value act_bwd_kernel's comparisons choose:
      relu          v > 0 ? 1 : 0                      -> 0 at 0 (the left derivative)
      hard_sigmoid  -3 < v < 3 ? 1/6 : 0               -> 0 at -3 and at 3 (the outer side)
      hard_swish    v <= -3 ? 0 : v >= 3 ? 1 : (2 v + 3) / 6  -> 0 at -3 (left; the right derivative is -1/2), 1 at 3 (right; the left
                    derivative is 3/2)"""
    x = np.asarray(x, F64)
    if act in (None, "none"):
        return np.ones_like(x)
    if act == "relu":
        return (x > 0).astype(F64)
    if act == "hard_sigmoid":
        return np.where((x > -3.0) & (x < 3.0), 1.0 / 6.0, 0.0)
    if act == "hard_swish":
        return np.where(x <= -3.0, 0.0, np.where(x >= 3.0, 1.0, (2.0 * x + 3.0) / 6.0))
    sg = 1.0 / (1.0 + np.exp(-x))
    if act == "sigmoid":
        return sg * (1.0 - sg)
    if act == "silu":
        return sg * (1.0 + x * (1.0 - sg))
    if act == "gelu_tanh":                               # y = x s(2 u): y' = s + x s (1 - s) 2 u'
        c = np.sqrt(2.0 / np.pi)
        u = c * (x + 0.044715 * x ** 3)
        s2 = 1.0 / (1.0 + np.exp(-2.0 * u))
        return s2 + x * s2 * (1.0 - s2) * 2.0 * c * (1.0 + 3.0 * 0.044715 * x * x)
    raise ValueError(act)


def layernorm_bwd64(x, gamma, dy, eps):
    """(dx, dy xhat) of y = xhat gamma + beta in float64: dx = rstd (g - mean(g) - xhat mean(g xhat)), g = gamma dy."""
    x, dy = np.asarray(x, F64), np.asarray(dy, F64)
    mean = x.mean(-1, keepdims=True)
    rstd = 1.0 / np.sqrt(((x - mean) ** 2).mean(-1, keepdims=True) + eps)
    xh = (x - mean) * rstd
    g = dy * (1.0 if gamma is None else np.asarray(gamma, F64))
    return rstd * (g - g.mean(-1, keepdims=True) - xh * (g * xh).mean(-1, keepdims=True)), dy * xh


def xent64(logits, target):
    """optax.softmax_cross_entropy(logits, target) per row, its mean, and the mean's gradient, in float64; the rows of `target` need
    not sum to 1: loss_b = ts_b lse_b - sum_k t l, dlogits = (ts softmax - t) / B."""
    l, t = np.asarray(logits, F64), np.asarray(target, F64)
    mx = l.max(-1, keepdims=True)
    lse = mx + np.log(np.exp(l - mx).sum(-1, keepdims=True))
    ts = t.sum(-1, keepdims=True)
    rows = (ts * lse - (t * l).sum(-1, keepdims=True))[:, 0]
    return rows, rows.mean(), (ts * np.exp(l - lse) - t) / l.shape[0]


def swin_bwd64(qkv, bias, dout, heads, ws, shift):
    """float64 autograd of the shifted-window attention core (tests/_cases.py: swin_bwd_case's `core`) for a rectangular map and
    window: roll, partition, q / sqrt(dh) . k + bias, the -100 mask between regions, softmax, reverse.  The shift of an axis whose
    window covers the map is dropped.  Returns (dqkv [B, Hf, Wf, 3 C], g [B nW, heads, n, n] = the gradient of the logits)."""
    B, Hf, Wf, C3 = qkv.shape
    C, (wh, ww) = C3 // 3, ws
    sh = [0 if wh >= Hf else shift[0], 0 if ww >= Wf else shift[1]]
    n, dh, nW = wh * ww, C // heads, (Hf // wh) * (Wf // ww)
    t = _t(qkv).requires_grad_(True)
    x = torch.roll(t, (-sh[0], -sh[1]), (1, 2)) if sum(sh) > 0 else t
    x = x.view(B, Hf // wh, wh, Wf // ww, ww, 3 * C).permute(0, 1, 3, 2, 4, 5).reshape(B * nW, n, 3, heads, dh).permute(2, 0, 3, 1, 4)
    q, k, v = x[0] * dh ** -0.5, x[1], x[2]
    attn = q @ k.transpose(-2, -1) + _t(bias)[None]
    if sum(sh) > 0:
        m = torch.zeros((Hf, Wf), dtype=torch.float64)
        c = 0
        for hh in ((0, -wh), (-wh, -sh[0]), (-sh[0], None)):
            for wl in ((0, -ww), (-ww, -sh[1]), (-sh[1], None)):
                m[hh[0]:hh[1], wl[0]:wl[1]] = c
                c += 1
        m = m.view(Hf // wh, wh, Wf // ww, ww).permute(0, 2, 1, 3).reshape(nW, n)
        m = m.unsqueeze(1) - m.unsqueeze(2)
        m = m.masked_fill(m != 0, -100.0)
        attn = (attn.view(B, nW, heads, n, n) + m[None, :, None]).view(-1, heads, n, n)
    attn.retain_grad()
    y = (attn.softmax(-1) @ v).transpose(1, 2).reshape(B * nW, n, C)
    y = y.view(B, Hf // wh, Wf // ww, wh, ww, C).permute(0, 1, 3, 2, 4, 5).reshape(B, Hf, Wf, C)
    if sum(sh) > 0:
        y = torch.roll(y, (sh[0], sh[1]), (1, 2))
    y.backward(_t(dout))
    return t.grad.numpy(), attn.grad.numpy()


# ================================================================================================ fused activations
# Instruments for the activations fused into the conv / GEMM epilogues and into se_scale (tests/test_strict_act_gpu.py, proofs in
# tests/test_strict_act_host.py).
#
# Exact instrument.  On a lattice of pre-activations every activation has an exactly representable value:
#     gelu_tanh                multiples of 16    ReLU              |t| = |x (k0 + k1 x^2)| >= 458 at |x| = 16
#     sigmoid / silu           multiples of 128   step / ReLU       |t| = log2(e) |x| >= 184
#     hard_sigmoid / _swish    multiples of 3     step / ReLU       fl(1/6) = (1/6)(1 + 2^-25): (6 v) fl(1/6) rounds back to v
# (step: 0 below 0, 1/2 at 0, 1 above).  Supposed of the hardware and not in the source: v_exp_f32(+-0) = 1, v_rcp_f32(1) = 1,
# v_rcp_f32(2) = 0.5, exp2 of an argument below -128 is below 2^-25 (1 + e rounds to 1), exp2 of an argument above 128 is +inf
# (rcp gives 0, and v * 0 = -0 for v < 0, which equals 0).  test_ln_mlp_exact rests on the same suppositions.  A lattice case that
# fails ONLY at pre-activation 0 for sigmoid / hard_sigmoid is a finding about the first three.
LATTICE_STEP = {"none": 1, "relu": 1, "gelu_tanh": 16, "hard_swish": 3, "hard_sigmoid": 3, "sigmoid": 128, "silu": 128}
STEP_ACTS = ("hard_sigmoid", "sigmoid")
TINY = 2.0 ** -126            # the smallest normal fp32 / bf16 value: what lies below it has no relative precision


def lattice_value(p, act):
    """What the activation is ON its lattice (float64; the caller proves that p is on it)."""
    p, act = np.asarray(p, F64), act_name(act)
    if act == "none":
        return p
    if act in STEP_ACTS:
        return np.where(p > 0, 1.0, np.where(p < 0, 0.0, 0.5))
    return np.maximum(p, 0.0)


def prove_lattice(name, pre, mag, act, weights, stored=(), out="bf16", signs=True, out_mag=None):
    """prove_exact's sibling for an activation beyond ReLU, asserted on the CPU before a launch.  `pre` is the float64
    pre-activation, `mag` its magnitude (the contraction on absolute values); returns the lattice value, the reference.
      (a) every pre-activation and every `mag` is a multiple of the activation's lattice step;
      (b) mag < 2^24 (fp32 accumulation exact in any order), 6 mag < 2^24 for the hard pair (v * h is exact);
      (c) a bf16 output holds the value: out_mag (default: mag) <= 256 at step 3 (the values 3 k are not all bf16 values beyond
          that), <= 256 steps at steps 1, 16 and 128; not asked of the step functions, whose values are 0, 1/2, 1;
      (d) every operand in `stored` is a bf16 value;
      (e) act64 rounded to the output type IS the lattice value (act64 itself is within 1e-50 of it, not on it);
      (f) prove_exact's coverage conditions on the weights;
      (g) signs: >= 5 % of the pre-activations negative, >= 5 % positive, at least one exactly 0."""
    act = act_name(act)
    step = LATTICE_STEP[act]
    pre, mag = np.asarray(pre, F64), np.asarray(mag, F64)
    for what, a in (("pre-activation", pre), ("mag", mag)):
        assert np.array_equal(np.rint(a / step) * step, a), f"{name}: {what} leaves the lattice of step {step}"
    top = float(mag.max())
    assert top < ACC_INT_MAX, f"{name}: mag reaches {top} >= 2^24"
    if step == 3:
        assert 6 * top < ACC_INT_MAX, f"{name}: 6 mag reaches {6 * top} >= 2^24"
    ref = lattice_value(pre, act)
    if out == "bf16" and act not in STEP_ACTS:
        otop = top if out_mag is None else float(np.abs(out_mag).max())
        lim = BF16_INT_MAX if step == 3 else BF16_INT_MAX * step
        assert otop <= lim, f"{name}: the output reaches {otop} > {lim} (not exact in bf16 at step {step})"
    for i, s in enumerate(stored):
        assert np.array_equal(bf(s), np.asarray(s, np.float32)), f"{name}: stored[{i}] is not a bf16 value"
    q = bf if out == "bf16" else (lambda a: np.asarray(a, np.float32))
    assert np.array_equal(q(act64(pre, act)).astype(F64), ref), f"{name}: act64 does not round to the lattice value"
    _prove_coverage(name, weights)
    if signs:
        neg, pos, zero = float((pre < 0).mean()), float((pre > 0).mean()), int((pre == 0).sum())
        assert neg >= 0.05 and pos >= 0.05 and zero >= 1, f"{name}: {100 * neg:.1f} % negative, {100 * pos:.1f} % positive, {zero} zeros"
    return ref


_LIPSCHITZ = {}


def act_lipschitz(act):
    """L = sup |act'| in float64, computed and not quoted: the analytic derivative (act_grad64) on a grid of step h = 2^-12 over
    [-12, 12] plus h / 2 max |act''| (from the grid's differences) for what lies between two grid points.  The hard pair is piecewise
    polynomial with corners at -3 and 3: each piece is taken with its own derivative on its CLOSED interval (1.5 at 3 for
    hard_swish comes from the middle piece).  Beyond +-12 the derivatives of sigmoid and silu tend monotonically to 0 / 0 and 1.
    gelu_tanh is tests/_strict_lngemm.py's gelu_lipschitz.  (1.5, 1/6, 0.25, 1.0998, 1.1290 for hard_swish, hard_sigmoid, sigmoid,
    silu, gelu_tanh: asserted to 1e-3 in tests/test_strict_act_host.py, as a check of this function only.)"""
    act = act_name(act)
    if act in _LIPSCHITZ:
        return _LIPSCHITZ[act]
    if act in ("none", "relu"):
        L = 1.0
    elif act == "gelu_tanh":
        from tests import _strict_lngemm
        L = _strict_lngemm.gelu_lipschitz()
    else:
        h = 2.0 ** -12
        if act == "hard_sigmoid":
            pieces = [(-3.0, 3.0, lambda x: np.full(x.shape, 1.0 / 6.0))]                 # 0 outside
        elif act == "hard_swish":
            pieces = [(-3.0, 3.0, lambda x: (2.0 * x + 3.0) / 6.0), (3.0, 12.0, lambda x: np.ones(x.shape))]
        else:
            pieces = [(-12.0, 12.0, lambda x: act_grad64(x, act))]
        L = 0.0
        for a, b, g in pieces:
            g1 = g(np.arange(a, b + 0.5 * h, h))
            L = max(L, float(np.abs(g1).max() + 0.5 * h * np.abs(np.diff(g1)).max() / h))
        if act in ("sigmoid", "silu"):
            lo, hi = act_grad64(np.array([-12.0, 12.0]), act)
            assert abs(lo) < 1e-3 and abs(hi - (act == "silu")) < 1e-3
    _LIPSCHITZ[act] = L
    return L


def through_act(p, e_p, act, out):
    """(ref, bound) of out(act(p)) for a float64 pre-activation p known to e_p (tests/_strict_lngemm.py's GELU line, for every
    activation):
        pre   = L e_p + n_ops(|p| + e_p) 2^-23 (|act(p)| + L e_p) + 2^-126
        bound = pre + half_ulp_out(|act(p)| + pre)                                   (out=None: pre alone, nothing is stored)
    L = act_lipschitz, n_ops = act_n_ops.  none / ReLU: L = 1 and n_ops = 0, so this is elem_bound.  The 2^-126 stands for the
    exponent range of fp32 (added for act >= 2 only): x rcp(1 + exp2(t)) is 0 once t > 128, where the function itself is below
    the smallest normal number."""
    act = act_name(act)
    p, e_p = np.asarray(p, F64), np.asarray(e_p, F64)
    L = act_lipschitz(act)
    ref = act64(p, act)
    pre = L * e_p + act_n_ops(np.abs(p) + e_p, act) * 2.0 ** -23 * (np.abs(ref) + L * e_p)
    if act not in ("none", "relu"):
        pre = pre + TINY
    return ref, (pre if out is None else pre + half_ulp_out(np.abs(ref) + pre, out))


def act_bound(p, mag, kred, act, out):
    """(ref, bound) of a conv / GEMM epilogue with activation `act`: e_p = (K_red + 4) 2^-23 mag as in elem_bound, then through_act."""
    return through_act(p, (kred + 4) * 2.0 ** -23 * np.asarray(mag, F64), act, out)


def prove_reach(name, p, act):
    """Gaussian pre-activations must reach the pieces of the function: >= 10 % in each of (-inf, -3), (-3, 3), (3, inf) for the hard
    pair; >= 10 % on each side of 0 and some |p| > 6 for gelu_tanh / sigmoid / silu."""
    act, p = act_name(act), np.asarray(p, F64)
    if act in ("hard_sigmoid", "hard_swish"):
        fr = [float((p < -3).mean()), float(((p > -3) & (p < 3)).mean()), float((p > 3).mean())]
        assert min(fr) >= 0.10, f"{name}: the pieces of {act} hold {fr} of the pre-activations"
    elif act in ("gelu_tanh", "sigmoid", "silu"):
        fr = [float((p < 0).mean()), float((p > 0).mean())]
        assert min(fr) >= 0.10 and bool((np.abs(p) > 6).any()), f"{name}: {fr} on the two sides of 0, max |p| {np.abs(p).max():.2f}"


# ------------------------------------------------------------------------------------------------ mv_se_scale_fwd (squeeze.hip)
SE_SHAPES = [(16, 4, 1), (72, 19, 5), (1032, 6, 67), (96, 33, 4 * 85 + 3)]         # (C, S, HW): what each reaches is in the GPU module
SE_ACTS = [("silu", "sigmoid"), ("relu", "hard_sigmoid"), ("none", "none")]
SE_N = 3


def se_groups(C):
    """se_scale_kernel's pooling passes: (first channel, end channel, cpb, pl) per group of up to 128 channel vectors."""
    c8 = C // 8
    return [(cv0 * 8, (cv0 + min(c8 - cv0, 128)) * 8, min(c8 - cv0, 128), 1024 // min(c8 - cv0, 128)) for cv0 in range(0, c8, 128)]


def se_data(mode, C, Sq, HW, act1, act2, bias, seed=80):
    """(x (3, HW, C), w1 (Sq, C), b1, w2 (C, Sq), b2); b1 = b2 = None without `bias`.
    gauss: bf16 Gaussians, every channel with an offset of its own so that the mean does not vanish.
    int:   x = a[n][c] + d[n][p][c], a in [-2, 2], d in [-2, 2] summing to 0 over the pixels (pairs +v, -v in a random order): the
           lane sums are small integers, the total is HW a, and (HW a) fl(1 / HW) == a is asserted in float32; +-1 rows (pm1_rows)
           times the lattice step of act1 for w1, +-1 (times the step of act2 unless act1's step is a multiple of it) for w2,
           biases integers times the step."""
    rng = rng_of(seed + C + 7 * HW + 1000 * (mode == "int") + ACT_CODES[act1])
    if mode == "gauss":
        x = bf(rng.standard_normal((SE_N, HW, C)) + 2.0 * rng.standard_normal((SE_N, 1, C)))
        w1, w2 = bf(rng.standard_normal((Sq, C)) / np.sqrt(C)), bf(rng.standard_normal((C, Sq)) / np.sqrt(Sq))
        b1, b2 = (0.5 * rng.standard_normal(Sq)).astype(F32), (2.0 * rng.standard_normal(C)).astype(F32)
        return x, w1, (b1 if bias else None), w2, (b2 if bias else None)
    s1, s2 = LATTICE_STEP[act1], LATTICE_STEP[act2]
    a = int_tensor(rng, (SE_N, 1, C), 2)
    v = int_tensor(rng, (SE_N, HW // 2, C), 2)
    d = rng.permuted(np.concatenate([v, -v, np.zeros((SE_N, HW % 2, C), F32)], axis=1), axis=1)
    x = (a + d).astype(F32)
    assert np.array_equal((F32(HW) * a[:, 0]) * (F32(1) / F32(HW)), a[:, 0]), "se: (HW a) fl(1 / HW) != a"
    w1 = F32(s1) * pm1_rows(rng, Sq, C, max(4, -(-C // Sq)))
    w2 = F32(1 if s1 % s2 == 0 else s2) * pm1_rows(rng, C, Sq, min(Sq, 2))
    b1, b2 = F32(s1) * int_tensor(rng, (Sq,), 4), F32(s2) * int_tensor(rng, (C,), 4)
    return x, w1, (b1 if bias else None), w2, (b2 if bias else None)


def se_ref(x, w1, b1, w2, b2, act1, act2):
    """The header's definition in float64 on the operands the kernel gets, with every term of the bound (counted from squeeze.hip):
      pooling   a lane adds ceil(HW / pl) pixels, min(pl, HW) lane sums are added in order (the other lanes hold exact zeros), the
                constant 1 / HW and the multiply: (ceil(HW / pl) + min(pl, HW) + 2) 2^-23 mean|x|
      fc1       ceil(C / 64) fma per lane, 6 shuffle adds, the bias add: (ceil(C / 64) + 7) 2^-23 mag1, plus |w1| . e_pool
      act1      through_act without a store (h stays in LDS as fp32)
      fc2       Sq fma starting from b2: Sq 2^-23 mag2, plus |w2| . e_h
      act2      through_act with the bf16 store.
    Returns {"q": pre-activation 1, "mq": its mag, "h", "r": pre-activation 2, "mr", "ref", "bound"}."""
    x, w1, w2 = np.asarray(x, F64), np.asarray(w1, F64), np.asarray(w2, F64)
    N_, HW, C = x.shape
    Sq = w1.shape[0]
    u = 2.0 ** -23
    p, pm = x.mean(1), np.abs(x).mean(1)
    n_pool = np.empty(C)
    for c0, c1, _, pl in se_groups(C):
        n_pool[c0:c1] = -(-HW // pl) + min(pl, HW) + 2
    e_pool = n_pool[None, :] * u * pm
    bb1 = 0.0 if b1 is None else np.asarray(b1, F64)
    bb2 = 0.0 if b2 is None else np.asarray(b2, F64)
    q = p @ w1.T + bb1
    mq = (np.abs(p) + e_pool) @ np.abs(w1).T + np.abs(bb1)
    e_q = e_pool @ np.abs(w1).T + (-(-C // 64) + 7) * u * mq
    h, e_h = through_act(q, e_q, act1, None)
    r = h @ w2.T + bb2
    mr = (np.abs(h) + e_h) @ np.abs(w2).T + np.abs(bb2)
    e_r = e_h @ np.abs(w2).T + Sq * u * mr
    ref, bound = through_act(r, e_r, act2, "bf16")
    return {"q": q, "mq": mq, "h": h, "r": r, "mr": mr, "ref": ref, "bound": bound}


def se_prove_exact(name, x, w1, b1, w2, b2, act1, act2):
    """Both pre-activations on their lattices (prove_lattice; h lives in LDS as fp32, the scale is stored as bf16 -- the limit of
    the bf16 store is asked of the reference values, fc2's partial sums are fp32).  Returns the exact reference."""
    pm = np.asarray(x, F64).mean(1)
    assert np.array_equal(pm, np.rint(pm)), f"{name}: the pooled means are not integers"
    q = pm @ np.asarray(w1, F64).T + (0.0 if b1 is None else np.asarray(b1, F64))
    mq = np.abs(pm) @ np.abs(np.asarray(w1, F64)).T + (0.0 if b1 is None else np.abs(np.asarray(b1, F64)))
    # 3 Sq hidden pre-activations are too few for the 5 % / exact-zero rule: both signs must occur; the rule is asked of fc2's
    h = prove_lattice(name + "/fc1", q, mq, act1, [w1], stored=[x, w1, w2], out="fp32", signs=False)
    assert bool((q < 0).any()) and bool((q > 0).any()), f"{name}: fc1's pre-activations have one sign"
    r = h @ np.asarray(w2, F64).T + (0.0 if b2 is None else np.asarray(b2, F64))
    mr = np.abs(h) @ np.abs(np.asarray(w2, F64)).T + (0.0 if b2 is None else np.abs(np.asarray(b2, F64)))
    ref = prove_lattice(name + "/fc2", r, mr, act2, [np.asarray(w2)], out="bf16", signs=act2 != "none", out_mag=lattice_value(r, act2))
    return ref


def emu_se_scale(x, w1, b1, w2, b2, act1, act2, store_mode="rne", lost_lane=False, w2_untransposed=False):
    """se_scale_kernel in float32, in its order: per channel group the pl pixel lanes (emu_global_avgpool), fc1 with lane c mod 64
    accumulating by fma and the xor-shuffle tree, + b1, act1; fc2 by fma from b2 over j, act2, the bf16 store.  Defects:
      lost_lane           the last pixel lane's sum is not added (the reduction stops at pl - 1)
      w2_untransposed     w2 is read as handed over by a caller that did not transpose it ([C][Sq] memory indexed as [Sq][C])"""
    x, w1, w2 = np.asarray(x, F32), np.asarray(w1, F32), np.asarray(w2, F32)
    N_, HW, C = x.shape
    Sq = w1.shape[0]
    pv = np.empty((N_, C), F32)
    for c0, c1, _, pl in se_groups(C):
        pv[:, c0:c1] = emu_global_avgpool(x[:, :, c0:c1], "fp32", pl=pl, lost_lane=pl - 1 if lost_lane else None)
    steps = -(-C // 64)
    wp, pp = np.zeros((Sq, steps * 64), F32), np.zeros((N_, steps * 64), F32)
    wp[:, :C], pp[:, :C] = w1, pv
    t = np.zeros((N_, Sq, 64), F32)
    for i in range(steps):
        sl = slice(64 * i, 64 * i + 64)
        t = (wp[None, :, sl].astype(F64) * pp[:, None, sl].astype(F64) + t.astype(F64)).astype(F32)
    for o in (32, 16, 8, 4, 2, 1):
        t = t + t[..., np.arange(64) ^ o]
    q = t[..., 0] + (F32(0) if b1 is None else np.asarray(b1, F32))
    h = act32(q, act1)
    w2t = np.ascontiguousarray(w2).reshape(Sq, C) if w2_untransposed else np.ascontiguousarray(w2.T)
    t = np.broadcast_to(np.zeros(C, F32) if b2 is None else np.asarray(b2, F32), (N_, C)).astype(F32)
    for j in range(Sq):
        t = (w2t[j][None, :].astype(F64) * h[:, j:j + 1].astype(F64) + t.astype(F64)).astype(F32)
    return store(act32(t, act2), "bf16", store_mode)
