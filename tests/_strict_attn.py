"""Strict instruments for the softmax attention kernels (tests/test_strict_attn_host.py, tests/test_strict_attn_gpu.py); numpy only.

Softmax outputs are not exactly representable in general, but the logits can be CHOSEN so that they are.  Every problem here is a
set of independent groups -- (image, head) for `mv_mha_*`, (image, window, head) for Swin -- of n queries / keys of width dh:
q, k, v (G, n, dh), an optional additive term `extra` (G, n, n) (relative-position bias + shift mask) and the logits
L = q . k^T * scale + extra.

Key codes.  code(j) is the low `nbits` bits of j as +-1, entry d carrying bit d % nbits; nbits = 8 for dh >= 32 (N <= 256), else the
bits N needs.  Two different keys differ in a bit that at least r = dh // nbits entries carry, so code(a) . code(b) <= dh - 2 r.
With q_i = g code(a) the logit of key a is g dh scale and every other one is at least 2 g r scale lower; `gain` takes the smallest
power of two g with 2 g r scale >= 128 (g = 64 for dh = 64, 128 for dh = 32): exp(-128) = 2.6e-56 is 0 in fp32 with or without
denormals, and every product and partial sum is an integer below 2^24 (exact in fp32 in any order).  Every construction is proved
on the CPU (`prove`) from float64 logits of the stored operands before a kernel output is looked at.

select   q_i = g code(pi(i)), pi a permutation per group (inside the query's mask region for Swin): ONE non-zero exponential pe.
         The MFMA kernels compute exp2(fma(s, sl2, -mx sl2)): pe = 1 + r with |r| <= 2^-14 (the rounding of mx sl2 < 2^11), bf16(pe) = 1
         exactly, the accumulator holds v[pi(i)] and the store rounds v (1 / pe) = v (1 - r) back to v (|r| << 2^-9): a bf16 output
         is BIT-EQUAL to v[pi(i)].  The returned probability is pe * rcp(pe): one reciprocal (1 ulp) and one product, within 2^-22 of
         1; the others are exactly 0.  The one-wave-per-query kernels subtract the maximum before __expf: pe = 1, fp32 outputs exact
         (asserted to 2^-21 relative).
tie      q_i = g (code(a_i) + code(b_i)), b_i = a_i with one bit flipped (bit 5: the other 32-key tile; bit 2: the other lane half
         of the accumulator layout, keys 4 fh + ...).  The two logits are the same integer, all others >= 128 lower; v integers in
         [-8, 8].  bf16(pe) = 1 twice, the accumulator holds v_a + v_b, the output (v_a + v_b) / 2 is a bf16 value: bit-equal.  The
         probabilities are pe * rcp(2 pe): within 2^-22 relative of 0.5.  A max or sum that is not exchanged between the lane halves,
         or a P . V step that pairs P with another key's V, cannot pass.
flat     q = -g, k = +1 (Swin: bias -400; on a shifted map the query's region at -400, the rest at -500, reference the region's
         mean): every real logit is -g dh scale <= -128; v integers in [-4, 4] + 3.  Reference S / N (S the integer column
         sum): bf16 within 2^-8 |S / N|, fp32 and the probabilities within (N + 8) 2^-24 relative (N - 1 additions, reciprocal,
         product).  A padded key that is not masked has logit 0, takes the maximum and sends the output to 0.
mask     (Swin) q = k = 0, bias 0, shifted windows: logits 0 inside the query's region, -100 outside; reference the mean of the
         integer v over the region; bound 2^-8 |mean| + 2^-100 (exp(-100) = 3.7e-44 is a denormal: flushed or not).
Swin form (a) selects by bias: q = k = 0, bias 0 at the winner(s) and -400 elsewhere (-400 everywhere for flat), so the gap stays
>= 128 where the -100 mask falls on the winner; tie pairs are taken from one mask class (same side of the shift boundary in both
axes), so that the mask treats them alike in every window.  Form (b) uses the codes with zero bias.

Gaussian bound (bf16 MFMA kernels), per element, with mag = sum_j p_j |v_j|, S = max_j (sum_d |q_d k_d| scale + |bias| + |mask|),
pe_j = exp(L_j - max L) and h(x) = 2^(floor(log2 x) - 8), the half ulp of a bf16 value (between 2^-9 x and 2^-8 x):
    e_p   = sum_j h(pe_j) |v_j| / sum_j pe_j     P rounded to bf16 before P . V (the denominator sums the unrounded pe)
    e_pre = e_p + n_ops 2^-24 mag,  n_ops = 2 (dh + 3) S + 2 N + 8:
            2 (dh + 3) S    a logit is dh accumulations, the scale constant and the multiply-add / bias / mask: dh + 3 roundings of S;
                            an absolute error e of a logit is a relative error e of its exponential, in the numerator and in the
                            denominator
            2 N + 8         the N-term sums of the denominator and of P . V; v_exp_f32 in both (4), v_rcp_f32 (2), the product with
                            1 / sum and the fold of log2(e) into the scale (2)
    bound = e_pre + h(|out| + e_pre)             the bf16 store
(h(.), not 2^-9 relative: that is the half ulp only at the top of a binade; the clean emulation exceeds 2^-9 mag + 2^-9 |out|.)
The fp32 / one-wave-per-query kernels do not round P: ops_bound with n_ops = 2 (dh + 3) S + 2 N + 8 (the form of the Swin V2 fp32
test).  Probabilities: the same n_ops relative to p.  On Gaussian v the sign of a P rounding error is random, so truncating P
stays inside any worst-case bound; it shows as the rounding BIAS of tests/_strict.py's instrument 2 (mean signed error in output
ulps: 0 for round-to-nearest, about -0.5 p_eff for truncation), which belongs to the Gaussian instrument here as it does there.

`emulate` is a float32 model of the MFMA kernels' arithmetic with one switch per defect (tests/test_strict_attn_host.py).
"""
from __future__ import annotations

import numpy as np

from tests import _strict as ST

F32, F64 = np.float32, np.float64
GAP = 128.0
DEFECTS = ("drop_last_key", "unmasked_pad", "swap_keys_in_step", "no_half_exchange", "truncate_p", "probs_unnormalised", "scale_off",
           "mask_region_off_by_one")


# ------------------------------------------------------------------------------------------------ codes
def nbits_of(N, dh):
    return 8 if dh >= 32 else max(1, int(np.ceil(np.log2(max(N, 2)))))


def codes(N, dh):
    """(N, dh) of +-1."""
    nb = nbits_of(N, dh)
    assert N <= (1 << nb) and dh >= nb, (N, dh)
    bit = np.arange(dh) % nb
    return np.where((np.arange(N)[:, None] >> bit[None, :]) & 1, 1.0, -1.0).astype(F32)


def gain(N, dh, scale):
    r = dh // nbits_of(N, dh)
    g = 2.0 ** np.ceil(np.log2(GAP / (2.0 * r * scale)))
    assert 2 * g <= 1024 and g * dh * 2 < ST.ACC_INT_MAX
    return float(g)


# ------------------------------------------------------------------------------------------------ constructions
def _perm_in_regions(rng, regions):
    """A permutation of the keys of every group that stays inside each region."""
    G, n = regions.shape
    pi = np.empty((G, n), np.int64)
    for g in range(G):
        for r in np.unique(regions[g]):
            idx = np.flatnonzero(regions[g] == r)
            pi[g, idx] = rng.permutation(idx)
    return pi


def _partner(a, i, n, ok, nb=8):
    """Key a with one code bit flipped: the other 32-key tile first, for every third query the other lane half first; a if none."""
    order = (2, 5, 0, 1, 3, 4, 6, 7) if i % 3 == 0 else (5, 2, 0, 1, 3, 4, 6, 7)
    for bit in order:
        b = a ^ (1 << bit)
        if bit < nb and b < n and ok(b):
            return b
    return a


def build(kind, G, n, dh, scale, seed, regions=None, by_bias=False, classes=None, heads=1):
    """One construction.  Returns a dict: q, k, v (G, n, dh) float32 (bf16 values), bias (heads, n, n) float32 or None, `win` (G, n, n)
    bool -- the keys that must share the maximum --, `expect` (G, n, dh) float64, and `regions` (G, n).
    by_bias: Swin form (a); the winners are per HEAD (group g has head g % heads), tie pairs from one mask class."""
    rng = ST.rng_of(seed)
    reg = np.zeros((G, n), np.int64) if regions is None else np.asarray(regions, np.int64)
    win = np.zeros((G, n, n), bool)
    ar = np.arange(n)
    c = codes(n, dh)
    g_ = gain(n, dh, scale)
    bias = None
    if kind == "select":
        v = ST.bf(rng.standard_normal((G, n, dh)))
    elif kind == "tie":
        v = ST.int_tensor(rng, (G, n, dh), 8)
    elif kind == "flat":
        v = ST.int_tensor(rng, (G, n, dh), 4) + F32(3)
    elif kind == "mask":
        v = ST.int_tensor(rng, (G, n, dh), 8)
    else:
        raise ValueError(kind)
    if kind in ("flat", "mask"):
        win = reg[:, :, None] == reg[:, None, :]              # all keys, or on a shifted map the query's region (flat: -400 / -500)
        if by_bias or kind == "mask":
            q = np.zeros((G, n, dh), F32)
            k = np.zeros((G, n, dh), F32)
            bias = np.full((heads, n, n), -400.0 if kind == "flat" else 0.0, F32)
        else:
            q = np.full((G, n, dh), -g_, F32)
            k = np.ones((G, n, dh), F32)
    elif by_bias:
        cls = np.zeros(n, np.int64) if classes is None else np.asarray(classes)
        bias = np.full((heads, n, n), -400.0, F32)
        q = np.zeros((G, n, dh), F32)
        k = np.zeros((G, n, dh), F32)
        for h in range(heads):
            pi = rng.permutation(n)
            w = np.zeros((n, n), bool)
            w[ar, pi] = True
            if kind == "tie":
                for i in range(n):
                    b = _partner(int(pi[i]), i, n, lambda t: cls[t] == cls[pi[i]])
                    if b == pi[i]:
                        same = np.flatnonzero((cls == cls[pi[i]]) & (ar != pi[i]))
                        b = int(same[i % same.size]) if same.size else b
                    w[i, b] = True
            bias[h][w] = 0.0
            win[h::heads] = w
    else:
        pi = _perm_in_regions(rng, reg)
        k = np.broadcast_to(c, (G, n, dh)).copy()
        q = g_ * c[pi]
        win[np.arange(G)[:, None], ar[None, :], pi] = True
        if kind == "tie":
            nb = nbits_of(n, dh)
            for g in range(G):
                for i in range(n):
                    a = int(pi[g, i])
                    b = _partner(a, i, n, lambda t: reg[g, t] == reg[g, a], nb)
                    win[g, i, b] = True
                    q[g, i] = g_ * (c[a] + c[b]) if b != a else 2 * g_ * c[a]
    v64 = v.astype(F64)
    cnt = win.sum(-1, keepdims=True)
    expect = (win.astype(F64) @ v64) / cnt
    if kind == "tie":
        assert (cnt == 2).mean() >= 0.5 and cnt.max() == 2, "tie: too few real ties"
    for a in (q, k, v):
        assert np.array_equal(ST.bf(a), a), "operands must be bf16 values"
    return {"kind": kind, "q": q.astype(F32), "k": k.astype(F32), "v": v.astype(F32), "bias": bias, "win": win, "expect": expect,
            "regions": reg, "scale": float(scale)}


def gauss(G, n, dh, scale, seed, dtype="bf16", heads=1, with_bias=False):
    rng = ST.rng_of(seed)
    qz = ST.q_of(dtype)
    q, k, v = (qz(rng.standard_normal((G, n, dh))).astype(F32) for _ in range(3))
    bias = (0.5 * rng.standard_normal((heads, n, n))).astype(F32) if with_bias else None
    return {"kind": "gauss", "q": q, "k": k, "v": v, "bias": bias, "scale": float(scale)}


# ------------------------------------------------------------------------------------------------ Swin geometry (numpy restatement)
def eff_shift(Hf, ws, shift):
    return 0 if ws >= Hf else shift


def hw(Hf):
    """A shape's map entry: Hf (square map) or (Hf, Wf)."""
    return (Hf, Hf) if np.isscalar(Hf) else tuple(Hf)


def region_map(Hf, ws, shift, off_by_one=False):
    """(nW, n) region ids of the rolled map: the mask construction of tests/_cases.py::_swin_core_ref.  off_by_one: the defect."""
    H, W = hw(Hf)
    nW, n = (H // ws) * (W // ws), ws * ws
    sh, sw = eff_shift(H, ws, shift), eff_shift(W, ws, shift)
    if sh == 0 and sw == 0:
        return np.zeros((nW, n), np.int64)
    m = np.zeros((H, W), np.int64)

    def bands(L, s):
        e = L - s + (1 if off_by_one else 0)
        return (0, L - ws), (L - ws, e), (e, L)

    c = 0
    for a in bands(H, sh):
        for b in bands(W, sw):
            m[a[0]:a[1], b[0]:b[1]] = c
            c += 1
    return m.reshape(H // ws, ws, W // ws, ws).transpose(0, 2, 1, 3).reshape(nW, n)


def mask_classes(Hf, ws, shift):
    """(n,) class of a window token: which side of the shift boundary in each axis (tokens of one class share a region in every window)."""
    H, W = hw(Hf)
    sh, sw = eff_shift(H, ws, shift), eff_shift(W, ws, shift)
    t = np.arange(ws * ws)
    return ((t // ws) >= ws - sh) * 2 + ((t % ws) >= ws - sw) if sh or sw else np.zeros(ws * ws, np.int64)


def swin_extra(bias, regions, heads, B):
    """(B nW heads, n, n) float64: bias + (-100 where the regions differ); groups ordered (image, window, head)."""
    nW, n = regions.shape
    am = np.where(regions[:, :, None] != regions[:, None, :], -100.0, 0.0)
    e = np.asarray(bias, F64)[None] + am[:, None]
    return np.broadcast_to(e[None], (B, nW, heads, n, n)).reshape(B * nW * heads, n, n)


def swin_pack(q, k, v, B, Hf, heads, ws, shift):
    """Groups (B nW heads, n, dh) -> qkv NHWC (B, Hf, Hf, 3 C), channel order [q | k | v][head][dh], the cyclic shift undone."""
    n, dh = q.shape[1:]
    H, W = hw(Hf)
    t = np.stack([q, k, v]).reshape(3, B, H // ws, W // ws, heads, ws, ws, dh)
    x = t.transpose(1, 2, 5, 3, 6, 0, 4, 7).reshape(B, H, W, 3 * heads * dh)
    return np.ascontiguousarray(np.roll(x, (eff_shift(H, ws, shift), eff_shift(W, ws, shift)), axis=(1, 2)))


def swin_groups(y, heads, ws, shift):
    """out NHWC (B, Hf, Hf, C) -> (B nW heads, n, dh)."""
    B, H, W, C = y.shape
    nh, nw, dh = H // ws, W // ws, C // heads
    x = np.roll(y, (-eff_shift(H, ws, shift), -eff_shift(W, ws, shift)), axis=(1, 2)).reshape(B, nh, ws, nw, ws, heads, dh)
    return x.transpose(0, 1, 3, 5, 2, 4, 6).reshape(B * nh * nw * heads, ws * ws, dh)


def mha_pack(q, k, v, B, H, head_major=False):
    """Groups (B H, N, dh) -> qkv [B, N, 3, H, dh] (as (B, N, 3 H dh)) or head-major [B, 3 H, N, dh]."""
    N, dh = q.shape[1:]
    t = np.stack([q, k, v]).reshape(3, B, H, N, dh)
    if head_major:
        return np.ascontiguousarray(t.transpose(1, 0, 2, 3, 4).reshape(B, 3 * H, N, dh))
    return np.ascontiguousarray(t.transpose(1, 3, 0, 2, 4).reshape(B, N, 3 * H * dh))


def mha_groups(y, H):
    """out (B, N, H dh) -> (B H, N, dh)."""
    B, N, D = y.shape
    return y.reshape(B, N, H, D // H).transpose(0, 2, 1, 3).reshape(B * H, N, D // H)


# ------------------------------------------------------------------------------------------------ float64 side
def logits64(p, extra=None):
    L = p["q"].astype(F64) @ p["k"].astype(F64).transpose(0, 2, 1) * p["scale"]
    return L if extra is None else L + extra


def prove(p, extra=None):
    """The host proof: the winners share the row maximum EXACTLY, every other key is >= 128 below (mask: exactly 100 below);
    flat: the common logit is <= -128 (an unmasked padding key at 0 would win by that much) unless the bias carries it."""
    L = logits64(p, extra)
    win = p["win"]
    top = np.where(win, L, -np.inf).max(-1, keepdims=True)
    assert np.isfinite(top).all() and win.any(-1).all(), "a query without a winner"
    assert (np.where(win, L, top) == top).all(), f"{p['kind']}: the winners' logits are not equal"
    rest = np.where(win, -np.inf, L).max(-1, keepdims=True)
    gap = 100.0 if p["kind"] in ("mask", "flat") else GAP      # flat on a shifted map: the mask's own -100
    assert (top - rest >= gap).all(), f"{p['kind']}: gap {float((top - rest).min())} < {gap}"
    if p["kind"] == "flat":
        assert (top <= -GAP).all(), "flat: a padding key at logit 0 would not win"
    assert np.abs(p["q"].astype(F64) @ p["k"].astype(F64).transpose(0, 2, 1)).max() < ST.ACC_INT_MAX
    return float((top - rest).min())


def ref64(p, extra=None):
    """(out, mag, smag, probs) in float64."""
    q, k, v = (p[t].astype(F64) for t in "qkv")
    L = logits64(p, extra)
    S = np.abs(q) @ np.abs(k).transpose(0, 2, 1) * p["scale"] + (0.0 if extra is None else np.abs(extra))
    pr = np.exp(L - L.max(-1, keepdims=True))
    pr = pr / pr.sum(-1, keepdims=True)
    return pr @ v, pr @ np.abs(v), S.max(-1, keepdims=True), pr


def p_round_mag(p, extra=None):
    """e_p of the module docstring: the worst case of rounding every exponential to bf16, as an error of the output."""
    L = logits64(p, extra)
    pe = np.exp(L - L.max(-1, keepdims=True))
    return (ST.half_ulp_out(pe, "bf16") @ np.abs(p["v"].astype(F64))) / pe.sum(-1, keepdims=True)


def n_ops(smag, n, dh):
    return 2.0 * (dh + 3) * smag + 2.0 * n + 8.0


def mfma_bound(ref, mag, smag, e_p, n, dh):
    e_pre = e_p + n_ops(smag, n, dh) * 2.0 ** -24 * mag
    return e_pre + ST.half_ulp_out(np.abs(ref) + e_pre, "bf16")


# ------------------------------------------------------------------------------------------------ checks (shared by host and GPU tests)
def check_exactish(kind, got, p, out="bf16", n=None):
    """select / tie: bf16 bit-equal, fp32 within 2^-21 relative.  flat / mask: within 2^-8 |ref| (+ 2^-100) for bf16, (N + 8) 2^-24 for
    fp32.  Returns tests/_strict-style info with "worst"."""
    ref = p["expect"]
    if kind in ("select", "tie"):
        if out == "bf16":
            info = ST.check_exact(got, ref)
            info["worst"] = "exact" if info["ok"] else "NOT exact"
            return info
        return ST.check_bound(got, ref, None, 0, out, bound=2.0 ** -21 * np.abs(ref))
    n = p["win"].shape[-1] if n is None else n
    extra_mask = not p["win"].all()                            # keys at -100: exp(-100) may or may not be flushed
    rel = 2.0 ** -8 if out == "bf16" else (n + 8) * 2.0 ** -24
    return ST.check_bound(got, ref, None, 0, out, bound=rel * np.abs(ref) + (2.0 ** -100 if extra_mask else 0.0))


def check_probs(kind, got, p, keepmask=None):
    """Probabilities of a construction: exactly 0 off the winners; on them within 2^-22 (relative) of 1 / #winners, (N + 8) 2^-24 for
    flat.  keepmask: dropped entries exactly 0, kept ones times 1 / keep."""
    win = p["win"]
    cnt = win.sum(-1, keepdims=True).astype(F64)
    ref = np.where(win, 1.0 / cnt, 0.0)
    if keepmask is not None:
        ref = ref * keepmask
    rel = (win.shape[-1] + 8) * 2.0 ** -24 if kind == "flat" else 2.0 ** -22
    return ST.check_bound(got, ref, None, 0, "fp32", bound=rel * ref)


def check_gauss(got, p, extra=None, out="bf16", mfma=True):
    """mfma: the per-element bound AND the rounding bias, which needs BIAS_MIN_ELEMS eligible elements (the Gaussian problems are
    sized for it: `gauss_shape`); too few is a failure, not a lapse of the check."""
    ref, mag, smag, _ = ref64(p, extra)
    n, dh = p["q"].shape[1:]
    if mfma:
        info = ST.check_bound(got, ref, mag, 0, "bf16", bound=mfma_bound(ref, mag, smag, p_round_mag(p, extra), n, dh))
        b, nb = ST.rounding_bias(got, ref, "bf16")
        info["bias"], info["n_bias"] = b, nb
        info["ok"] = bool(info["ok"] and nb >= ST.BIAS_MIN_ELEMS and abs(b) <= ST.BIAS_LIMIT)
        return info
    return ST.check_bound(got, ref, mag, 0, out, n_ops=np.broadcast_to(n_ops(smag, n, dh), ref.shape))


def check_gauss_probs(got, p, extra=None):
    _, _, smag, pr = ref64(p, extra)
    n, dh = p["q"].shape[1:]
    return ST.check_bound(got, pr, None, 0, "fp32", bound=n_ops(smag, n, dh) * 2.0 ** -24 * pr)


def old_cmp(got, ref, tol):
    """tests/_cases.py::_cmp, the criterion these instruments replace: max |got - ref| <= tol max(1, max |ref|)."""
    got, ref = np.asarray(got, F64), np.asarray(ref, F64)
    return bool(np.isfinite(got).all() and np.abs(got - ref).max() <= tol * max(1.0, np.abs(ref).max()))


# ------------------------------------------------------------------------------------------------ emulator
def emulate(p, extra=None, n_pad=None, keepmask=None, **defect):
    """float32 model of the MFMA kernels: fp32 logits, the padded keys masked, exp of the difference to the maximum, P rounded to
    bf16, fp32 accumulation of P . V, the product with 1 / sum, a bf16 store.  Returns (out (G, n, dh), probs (G, n, n)).
    One defect per switch:
      drop_last_key       key n - 1 is masked like a padded key
      unmasked_pad        one padded key (if there is one) keeps its logit 0
      swap_keys_in_step   two keys of one k16 step exchanged on the V side only
      no_half_exchange    1 / sum from the keys of one lane half ((key >> 2) & 1) only: the half that stores the channel / probability
      truncate_p          P truncated to bf16
      probs_unnormalised  the returned probabilities are the exponentials
      scale_off           scale * 1.02
    (mask_region_off_by_one is a switch of region_map: it changes `extra`.)"""
    unknown = set(defect) - set(DEFECTS)
    assert not unknown, unknown
    q, k, v = (np.asarray(p[t], F32) for t in "qkv")
    G, n, dh = q.shape
    NP = n_pad or 32 * -(-n // 32)
    kp = np.zeros((G, NP, dh), F32)
    vp = np.zeros((G, NP, dh), F32)
    kp[:, :n], vp[:, :n] = k, v
    sc = F32(p["scale"] * (1.02 if defect.get("scale_off") else 1.0))
    L = (q @ kp.transpose(0, 2, 1)) * sc
    if extra is not None:
        L[:, :, :n] = L[:, :, :n] + np.asarray(extra, F32)
    masked = np.arange(NP) >= n
    if defect.get("unmasked_pad") and NP > n:
        masked[n] = False
    if defect.get("drop_last_key"):
        masked[n - 1] = True
    L[:, :, masked] = -np.inf
    with np.errstate(under="ignore"):
        pe = np.exp(L - L.max(-1, keepdims=True)).astype(F32)
    half = (np.arange(NP) >> 2) & 1
    if defect.get("no_half_exchange"):
      with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
        sums = np.stack([pe[:, :, half == h].sum(-1, dtype=F32) for h in (0, 1)], -1)          # (G, n, 2)
        inv = F32(1) / sums
        inv_key, inv_d = inv[:, :, half], inv[:, :, (np.arange(dh) >> 2) & 1]
    else:
        inv = (F32(1) / pe.sum(-1, dtype=F32))[:, :, None]
        inv_key, inv_d = inv, inv
    if keepmask is not None:
        km = np.zeros((G, n, NP), F32)
        km[:, :, :n] = keepmask
        pe = pe * km
    with np.errstate(invalid="ignore", over="ignore"):
        probs = (pe if defect.get("probs_unnormalised") else pe * inv_key)[:, :, :n]
    P = ST.bf16_truncate(pe) if defect.get("truncate_p") else ST.bf(pe)
    if defect.get("swap_keys_in_step"):
        j0 = (n - 1) & ~15
        j0 = j0 if j0 + 1 < n else 0
        vp[:, [j0, j0 + 1]] = vp[:, [j0 + 1, j0]]
    with np.errstate(invalid="ignore", over="ignore"):
        out = ST.bf((P @ vp).astype(F32) * inv_d)
    return out, probs


# ------------------------------------------------------------------------------------------------ the shapes of the GPU tests
MHA_SHAPES = ((2, 197, 3, 64), (1, 33, 1, 64), (2, 256, 2, 32), (1, 17, 2, 32), (1, 225, 2, 32))          # (B, N, H, dh)
MHA_HM_SHAPES = ((2, 197, 3, 64), (1, 33, 2, 32))
MHA_DROP_SHAPES = ((2, 197, 3, 64, False), (1, 33, 1, 64, True))                                         # (.., head_major)
MHA_OTHER = ((1, 197, 2, 64, "bf16", True, "mha_generic"), (1, 8, 4, 8, "bf16", False, "mha_generic"),   # (.., dtype, force_generic, kernel)
             (1, 50, 2, 16, "fp32", False, "mha_generic"), (16, 50, 8, 16, "fp32", False, "mha_f32_lds"))
SWIN_SHAPES = ((2, 14, 96, 3, 7, 3), (2, 14, 96, 3, 7, 0), (1, 7, 192, 6, 7, 3), (2, 16, 64, 2, 8, 4), (2, 12, 64, 2, 4, 2))   # (B, Hf, C, heads, ws, shift)
SWIN_OTHER = ((2, 14, 96, 3, 7, 3, "bf16", True, "swin_attn_generic"), (1, 14, 32, 2, 7, 3, "fp32", False, "swin_attn_f32_lds"))
COS_SHAPES = ((1, 14, 64, 2, 7, 3), (1, 16, 64, 2, 8, 4))
# Hf = (Hf, Wf): the window covers the map in one axis (its shift is dropped), the other wraps at the largest legal shift, ws - 1
SWIN_WRAP_SHAPES = ((1, (8, 4), 32, 1, 4, 3), (1, (4, 8), 32, 1, 4, 3))


def swin_problem(kind, shape, seed, by_bias=True, off_by_one=False, dtype="bf16"):
    """(problem, extra, regions) of a Swin shape; `extra` = bias + mask from region_map (off_by_one: the defective mask)."""
    B, Hf, C, heads, ws, shift = shape
    n, dh = ws * ws, C // heads
    nW = (hw(Hf)[0] // ws) * (hw(Hf)[1] // ws)
    reg = region_map(Hf, ws, shift)
    G = B * nW * heads
    greg = np.broadcast_to(reg[None, :, None], (B, nW, heads, n)).reshape(G, n)
    scale = dh ** -0.5
    if kind == "gauss":
        p = gauss(G, n, dh, scale, seed, dtype, heads, with_bias=True)
    else:
        p = build(kind, G, n, dh, scale, seed, regions=greg, by_bias=by_bias, classes=mask_classes(Hf, ws, shift), heads=heads)
    bias = np.zeros((heads, n, n), F32) if p["bias"] is None else p["bias"]
    p["bias"] = bias
    extra = swin_extra(bias, region_map(Hf, ws, shift, off_by_one), heads, B)
    return p, extra


def gauss_shape(shape):
    """The mha shape of the Gaussian case: the same (N, H, dh) with B raised until B H N dh >= 8192, so that the rounding bias has
    its 4096 elements of |ref| >= 2^-6 at the one-tile and one-key-in-the-last-tile shapes too."""
    B, N, H, dh = shape[:4]
    return (max(B, -(-8192 // (N * H * dh))),) + tuple(shape[1:])


def mha_problem(kind, shape, seed, dtype="bf16"):
    """kind "gauss": pass gauss_shape(shape)."""
    B, N, H, dh = shape
    if kind == "gauss":
        return gauss(B * H, N, dh, dh ** -0.5, seed, dtype)
    return build(kind, B * H, N, dh, dh ** -0.5, seed)


def expect_dropped(p, keepmask):
    """The construction's expected output under attention dropout: the winners' weights 1 / #winners times keepmask (0 or 1 / keep)."""
    cnt = p["win"].sum(-1, keepdims=True).astype(F64)
    return ((p["win"] * keepmask) @ p["v"].astype(F64)) / cnt
