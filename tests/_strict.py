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


def check_bound(got, ref, mag, kred, out):
    got, ref = np.asarray(got, F64), np.asarray(ref, F64)
    if got.shape != ref.shape:
        return {"ok": False, "err": f"shape {got.shape} vs {ref.shape}"}
    if not np.isfinite(got).all():
        return {"ok": False, "err": "non-finite output", "nan": int((~np.isfinite(got)).sum())}
    b = elem_bound(ref, mag, kred, out)
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
