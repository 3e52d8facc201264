"""Strict instruments for the concat-free conv kernels -- mv_fire_expand_fwd, mv_conv3x3_pair_fwd, mv_conv3x3_slice_fwd (csrc/flat3x3.h)
and mv_conv1x1_split_fwd, mv_preact_conv1x1_fwd (csrc/pw128.h): case tables, data builders, float64 references with `mag`,
per-element bounds and numpy / float32 emulations of the five contracts, one defect switch each.  Used by
tests/test_strict_concat_gpu.py (the launches) and tests/test_strict_concat_host.py (the CPU proofs that the instruments see each
seeded defect).  The instruments themselves are tests/_strict.py's: prove_exact, check_exact, check_bound, check_bias.

Every builder returns a dict `d`: the operands as the kernel takes them (the 3x3 filters as PACKED FRAGMENTS, ops.fire_fragments /
ops.inception_fragments), the destinations ((rows, ld) each, sentinel-filled with a guard behind them) and `slices`: (destination,
first column, float64 reference, bound or None).  An emulation returns the flat destinations; `verdict` judges them -- the guard, the
sentinel outside the slices, no non-finite value, then per slice bit equality (modes "int" and "round") or the bound and, where
the project's condition holds on the REFERENCE (bf16 output, kred <= 1152, >= 4096 elements with |ref| >= 2^-6), the rounding bias.

The fragment layout the 3x3 emulations decode (flat3x3.h): [tile][k-step][64 lanes][8]; lane L of k-step ks of a tile holds output
channel mfma32_tile_row(L % 32) of the tile and reduction indices 16 ks + 8 (L / 32) .. + 7, the reduction index being tap * S + c
(a k-step is 16 channels of ONE tap); the second tile of a pair is the next tile, 9 KC * 64 entries behind the first.  The reference
never sees the fragments: it is torch's float64 conv2d on the plain KRSC filter, so a packer that disagrees with the layout fails.
Accumulation: whole 16-channel k-steps in fp32, taps in order; pointwise: 64-channel chunks of 16-channel k-steps.  Store: pack_bf2,
round-to-nearest-even.

Instrument 1 (mode "int").  Activations in [-2, 2], S.pm1_rows weights, S.int_scale scales, integer shifts / biases;
S.prove_exact before any launch; per case ReLU is exercised on both sides (identity stores: negatives occur).  preact: s1 from
S.int_scale, integer h1, `a` an integer (a quarter-integer under pool 2: frac_bits = 2, s1 in {+-1}, |h1| <= 1) listed in `hidden`.

Instrument 1b (mode "round").  The same integers plus a carrier: reduction index (centre tap, channel 0) has weight +-64 in every
output row and activation 9 .. 14 at every pixel, the rest is 4 weights of +-1 per row, scales +-1, |shift| <= 8: every pre-store
value is an integer in [512, 1024), where bf16 keeps multiples of 4.  Residue 2 is an exact tie (25 %), residues 3 and 6 mod 8 differ
under truncation (37.5 %); under ReLU one channel in eight has a negative carrier.  Reference S.bf(ref64).  One case per store
path: fire_store, store16_relu via pair and split, store16_plain via slice and the preact transition (pool 2 on a map whose 2 x 2
windows are constant, so the means are the integers themselves).

Instrument 2 (mode "gauss").  N(0, 1) activations and N(0, 1 / kred) weights rounded to bf16, S.gauss_scale, N(0, 1) shifts.
fire / pair / slice / split: S.elem_bound(ref, mag, kred, "bf16"), kred = 9 S (3x3), S (Fire's 1x1 half), C (pointwise).
preact (reference with `a` UNROUNDED in float64), counted from preact_acc8 / PreactRows::stash:
    n_a   = 1 (pool 1: the fma; the add to 0 is exact)  |  4 (pool 2: the four fmas count once against the window's mean of
            |x s1| + |h1|, three inexact adds of partial sums <= 4 mag_a, `* 0.25f` exact)
    mag_a = mean_window(|x s1| + |h1|)            e_a = n_a 2^-23 mag_a + half_ulp_bf16(|a| + n_a 2^-23 mag_a)
    E     = e_a |W|^T                             mag = ((|a| + e_a) |W|^T) |s2| + |h2|
    e_pre = E |s2| + (C + 4) 2^-23 mag            bound = e_pre + half_ulp_bf16(|ref| + e_pre)

Worst |got - ref| / bound over all Gaussian cases (the GPU ratio is <= 1 by construction of the bound, not a tuned number):
    kernel      CPU emulation   MI355X      largest |rounding bias| on the MI355X (limit 0.05)
    fire        0.999           0.999       0.006
    pair        0.988           0.988       0.010
    slice       0.989           0.989       0.002
    split       0.996           0.996       0.004
    preact      0.700           0.700       0.026
(the four plain kernels sit at the store's half ulp, which is nearly all of their bound, so a violation by a hair is first to be read
as another legitimate summation order; preact's bound carries the rounding of `a`.)  On the MI355X all 128 cases passed: no element
differed in modes "int" / "round", none violated its bound, every kernel name, sentinel and guard held, and no kernel, gate or
packer had to be changed.

Seeded defects (emulation switches; tests/test_strict_concat_host.py proves each rejected at the shapes of REJECTED_AT):
  flat range   neighbour_image            the h test of a tap is lost: the tap reads flat pixel m + dh W + dw of the next / previous image.
                                          Needs B > 1 (or a neighbouring row of the range); invisible on a single image.
               row_wrap                   only the h test is kept: a tap past the row's end reads the neighbouring row.
               halo_not_zero_past_M       NOT REJECTED, by construction: range slots past M are read only by a tap that passed its image
                                          test, and the last pixel of the last image is M - 1; the defect is an out-of-bounds READ of the
                                          source, which no value check can see (the zeros past M are a second line of defence).
               swap_rs                    the filter is transposed.  Invisible on 1 x 1 maps (the centre tap alone is inside).
               drop_kstep (tap, kc)       invisible where the tap is outside every pixel's map (corner taps at H = 1 or W = 1).
               last_prefetch_repeat       step KS - 2 uses the fragment of step KS - 1.  KS - 2 is tap (2, 1) at KC = 1, else tap
                                          (2, 2): invisible where that tap is outside the map (H = 1; W = 1 unless KC = 1).
  tiles        upper_half_stored          N % 32 == 16: the zero rows' 16 channels are written behind the slice -> the sentinel check.
               second_tile_of_odd_count   the single last tile takes its fragments from the partner's place (past the array: zeros).
               pair_uses_S0_pitch         convolution 1 reads its slice from ct0 (NaN or the other slice's channels).
  epilogue     trunc, half_up             the store truncates / rounds half away from zero: mode "round", and the bias rule.
               shift_from=16              the shift of channel n + 16.  Invisible at N = 16 (one group: nothing else to read but OOB).
               relu_before_affine         visible only through a negative scale (S.int_scale / S.gauss_scale: every fifth at least).
               bias_of_other_half         Fire: b1 and b3 trade places.       null_bias_reads_b1   Fire: a null b3 reads b1.
  pw128.h      drop_last_partial_chunk    C % 64 != 0.      stale_buffer   chunk ch reads chunk ch - 2's buffer: C = 144.
               dead_wave_stores           the wave whose 64 columns are past N stores its zeros: sentinel check (destinations have room).
               n0_group_to_dst0           the group at n0 lands behind slice 0: sentinel check, and slice 1 keeps its sentinel.
  preact       round_before_mean          NOT REJECTED by the three modes: in modes "int" / "round" every relu(fma) is already a bf16
                                          value, and on Gaussian data the extra rounding (<= half_ulp(max r)) stays inside e_a |W|^T, a
                                          worst-case sum.  `preact_mean_case` closes it: four values = 3 mod 4 in [257, 511] with a mean
                                          = 2 mod 4 -- exact when averaged first, two off when rounded first -- through one +-1 weight.
               pool_pitch_2Wo             the source row pitch is 2 Wo: odd W only.
               relu_dropped_in_front, s1_abs
               read_past_C                NOT REJECTED with NaN behind C, three times over: k-steps past C are not run, the weight
                                          rows past C are zeros in LDS, and fmaxf(NaN, 0) = 0 launders the NaN in front of them.  The
                                          switch models all three masks lost (C rounded up to the chunk, the next row's weights read);
                                          the data therefore keeps NaN in channels C .. C + 7 and puts 2^14 in C + 8 .. C + 15, which
                                          the switch does turn into wrong values.
"""
from __future__ import annotations

import functools

import numpy as np

from eqxvision_amd import ops
from tests import _strict as S

F32, F64 = np.float32, np.float64
SENTINEL = -7.0               # tests/_slices.py
GUARD = 64
POISON = 2.0 ** 14            # behind C in preact's source rows, next to the NaN (module docstring: read_past_C)
FLAT_LDS_MAX = 160 * 1024
FIRE_LDS_TWO = 64 * 1024


def tile_row(p):
    """flat3x3.h, mfma32_tile_row: the output channel (inside its 32-channel tile) that row p of an A tile holds."""
    return 16 * ((p >> 2) & 1) + 4 * (p >> 3) + (p & 3)


def flat_lds_bytes(TM, W, S_):
    return (TM + 2 * W + 3) * (2 * S_ + 16)


def decode_fragments(frag, taps):
    """[tile][k-step][64][8] -> the filter [32 tiles][taps][S] by the layout the header states (restated here, not imported)."""
    frag = np.asarray(frag, F32)
    T, KS = frag.shape[:2]
    assert frag.shape[2:] == (64, 8) and (KS * 16) % taps == 0
    wk = np.full((T, 32, KS, 16), np.nan, F32)
    for lane in range(64):
        wk[:, tile_row(lane % 32), :, 8 * (lane // 32):8 * (lane // 32) + 8] = frag[:, :, lane, :]
    assert not np.isnan(wk).any()
    return wk.reshape(T * 32, taps, KS * 16 // taps)


def pack3x3(w_krsc, s_pad=None):
    """ops.inception_fragments of a KRSC filter (the packers take [N][S][kh][kw])."""
    return ops.inception_fragments(np.ascontiguousarray(np.asarray(w_krsc, F32).transpose(0, 3, 1, 2)), s_pad)


# ------------------------------------------------------------------------------------------------ stores and destinations
def store_bf(y, mode="rne"):
    y = np.ascontiguousarray(np.asarray(y, F32))
    if mode == "rne":
        return S.bf(y)
    if mode == "trunc":
        return S.bf16_truncate(y)
    assert mode == "half_up"
    return ((y.view(np.uint32) + np.uint32(0x8000)) & np.uint32(0xffff0000)).view(F32)


def _store_mode(defect):
    return defect if defect in ("trunc", "half_up") else "rne"


def new_dest(M, ld):
    return np.full(M * ld + GUARD, SENTINEL, F32)


def put(buf, ld, col, vals):
    """vals (M, n) to flat index m * ld + col + j, as a kernel writes: a column past the row lands in the next row or the guard."""
    vals = np.asarray(vals, F32)
    idx = np.arange(vals.shape[0])[:, None] * ld + col + np.arange(vals.shape[1])[None, :]
    keep = idx < buf.size
    buf[idx[keep]] = vals[keep]


def _fma(a, s, h):
    return (np.asarray(a, F64) * np.asarray(s, F64) + np.asarray(h, F64)).astype(F32)


def _padded(v, n):
    o = np.zeros(n, F32)
    o[:len(v)] = v
    return o


def epi_relu(acc, scale, shift, defect=None):
    """store16_relu: pack_bf2(fmaxf(fmaf(a, scale, shift), 0))."""
    sc, sh = _padded(scale, acc.shape[1]), _padded(shift, acc.shape[1])
    if defect == "shift_from":
        sh = np.roll(sh, -16)
    if defect == "relu_before_affine":
        v = _fma(np.maximum(acc, F32(0)), sc, sh)
    else:
        v = np.maximum(_fma(acc, sc, sh), F32(0))
    return store_bf(v, _store_mode(defect))


# ------------------------------------------------------------------------------------------------ the flat-range 3x3 product
def flat_acc(t2, ct, S_, frag, H, W, taps=9, defect=None, arg=None):
    """fp32 accumulators (M, 32 tiles) of flat_stage + flat_tap_offsets + flat_taps9 on the rows t2 (M, ldt) of flattened pixels."""
    M = t2.shape[0]
    wd = decode_fragments(frag, taps)
    Np, KC = wd.shape[0], S_ // 16
    assert wd.shape[2] == S_
    if defect == "second_tile_of_odd_count" and (Np // 32) % 2:
        wd = wd.copy()
        wd[-32:] = 0
    m = np.arange(M)
    rem = m % (H * W)
    h, w = rem // W, rem % W
    steps = [(tp, kc) for tp in range(taps) for kc in range(KC)]
    acc = np.zeros((M, Np), F32)
    for i, (tp, kc) in enumerate(steps):
        if defect == "drop_kstep" and (tp, kc) == tuple(arg):
            continue
        r, s = (tp // 3, tp % 3) if taps == 9 else (1, 1)
        if defect == "swap_rs":
            r, s = s, r
        dh, dw = r - 1, s - 1
        idx = m + dh * W + dw
        ok_h, ok_w = (h + dh >= 0) & (h + dh < H), (w + dw >= 0) & (w + dw < W)
        use = ok_w if defect == "neighbour_image" else ok_h if defect == "row_wrap" else ok_h & ok_w
        inr = (idx >= 0) & (idx < M)
        val = t2[np.clip(idx, 0, M - 1), ct + 16 * kc:ct + 16 * kc + 16]
        val = np.where(inr[:, None], val, F32(3.0 if defect == "halo_not_zero_past_M" else 0.0))
        xt = np.where(use[:, None], val, F32(0)).astype(F32)
        tj, kj = steps[i + 1] if defect == "last_prefetch_repeat" and i == len(steps) - 2 else (tp, kc)
        acc = acc + xt @ wd[:, tj, 16 * kj:16 * kj + 16].T
    return acc


FLAT_DEFECTS = ("neighbour_image", "row_wrap", "halo_not_zero_past_M", "swap_rs", "drop_kstep", "last_prefetch_repeat",
                "second_tile_of_odd_count")


def _flat(defect):
    return defect if defect in FLAT_DEFECTS else None


# ------------------------------------------------------------------------------------------------ verdict
def verdict(d, bufs, mode):
    """Judges the flat destinations of an emulation or of the GPU: {"ok", "why", "worst", "bias", "wrong"}."""
    why, worst, biases, wrong = [], 0.0, [], 0
    for i, (M, ld) in enumerate(d["dests"]):
        b = np.asarray(bufs[i], F64)
        rows, guard = b[:M * ld].reshape(M, ld), b[M * ld:]
        if guard.size != GUARD or not (guard == SENTINEL).all():
            why.append(f"dest {i}: guard overwritten")
        own = np.zeros(ld, bool)
        for j, c, ref, _ in d["slices"]:
            if j == i:
                own[c:c + ref.shape[1]] = True
        if not np.isfinite(rows).all():
            why.append(f"dest {i}: {int((~np.isfinite(rows)).sum())} non-finite values")
        if not (rows[:, ~own] == SENTINEL).all():
            why.append(f"dest {i}: written outside the slices at columns {np.unique(np.argwhere(rows[:, ~own] != SENTINEL)[:, 1])[:8].tolist()}"
                       " (of the columns not owned)")
    for k, (j, c, ref, bound) in enumerate(d["slices"]):
        M, ld = d["dests"][j]
        got = np.asarray(bufs[j], F64)[:M * ld].reshape(M, ld)[:, c:c + ref.shape[1]]
        if mode != "gauss":
            e = S.check_exact(got, ref)
            wrong += e.get("nbad", ref.size)
            if not e["ok"]:
                why.append(f"slice {k}: {e}")
            continue
        a = S.check_bound(got, ref, None, None, "bf16", bound=bound)
        worst = max(worst, a.get("worst", np.inf))
        if not a["ok"]:
            why.append(f"slice {k} bound: {a}")
        if bias_applies(ref, d["kred"][k]):
            bi = S.check_bias(got, ref, "bf16")
            biases.append(bi["bias"])
            if not bi["ok"]:
                why.append(f"slice {k} bias: {bi}")
    return {"ok": not why, "why": why, "worst": worst, "bias": biases, "wrong": wrong}


def bias_applies(ref, kred):
    return kred <= S.BIAS_MAX_KRED and int((np.abs(ref) >= 2.0 ** -6).sum()) >= S.BIAS_MIN_ELEMS


# ------------------------------------------------------------------------------------------------ operands
def _sparse_pm1(rng, rows, kred, nnz):
    w = np.zeros((rows, kred), F32)
    for r in range(rows):
        pos = rng.choice(kred, nnz, replace=False)
        w[r, pos] = rng.choice(np.array([-1.0, 1.0], F32), nnz)
    return w


def _weights(rng, mode, rows, kred, carrier, nnz_max, relu):
    """(rows, kred).  int: pm1_rows with every reduction index used; round: 4 of +-1 and the carrier +-64 (negative for one row in
    eight under ReLU, for every other row else); gauss: N(0, 1 / kred) in bf16."""
    if mode == "gauss":
        return S.bf(rng.standard_normal((rows, kred)) / np.sqrt(kred)), None
    if mode == "int":
        nnz = max(-(-kred // rows), min(8, kred))
        assert nnz <= nnz_max, f"nnz {nnz} > {nnz_max}: mag would pass 256"
        return S.pm1_rows(rng, rows, kred, nnz), None
    w = _sparse_pm1(rng, rows, kred, 4)
    sign = np.where(np.arange(rows) % (8 if relu else 2) == 1, -1.0, 1.0).astype(F32)
    w[:, carrier] = 64.0 * sign
    return w, sign


def _acts(rng, mode, shape):
    if mode == "gauss":
        return S.bf(rng.standard_normal(shape))
    x = S.int_tensor(rng, shape, 2)
    if mode == "round":
        x[..., 0] = rng.integers(9, 15, shape[:-1])
    return x


def _scale_shift(rng, mode, n, sign=None):
    if mode == "gauss":
        return S.gauss_scale(rng, n), rng.standard_normal(n).astype(F32)
    if mode == "round":                              # +-1, and the carrier's sign goes with it so that the product stays positive
        sc = S.int_scale(rng, n, (1,))
        return sc, S.int_tensor(rng, (n,), 8)
    return S.int_scale(rng, n), S.int_tensor(rng, (n,), 8)


def _rows_with_pad(x, pad, poison=np.nan):
    """(..., C) -> (..., C + pad) with what must never be read behind C."""
    if not pad:
        return np.ascontiguousarray(x, F32)
    return np.concatenate([x, np.full(x.shape[:-1] + (pad,), poison, F32)], -1).astype(F32)


def _both_sides(name, pre, relu):
    pre = np.asarray(pre)
    assert (pre < 0).any() and (pre > 0).any(), f"{name}: the pre-store values have one sign only"
    if relu:
        assert (pre < 0).mean() > 0.02, f"{name}: ReLU is hardly exercised"


def _round_preconditions(name, pre, relu):
    """Mode "round": integers of magnitude < 1024 that bf16 cannot hold; the tie and truncation shares of ALL outputs."""
    v = np.maximum(pre, 0.0) if relu else np.asarray(pre, F64)
    assert np.array_equal(v, np.rint(v)) and np.abs(v).max() < 1024, name
    r = S.bf(v).astype(F64)
    ties = np.abs(r - v) == S.half_ulp_out(np.abs(v), "bf16")
    ties &= r != v
    diff = S.bf16_truncate(v.astype(F32)).astype(F64) != r
    assert ties.mean() >= 0.10, f"{name}: {100 * ties.mean():.1f} % exact ties"
    assert diff.mean() >= 0.25, f"{name}: {100 * diff.mean():.1f} % differ under truncation"
    return r


def _finish3x3(name, mode, x4, w_krsc, scale, shift, relu, kred, nnz_note=None):
    """(ref, bound or None) of one 3x3 convolution (pad 1) in float64; the mode's preconditions asserted."""
    ref, mag, pre = S.conv_ref(x4, w_krsc, scale, shift, None, "relu" if relu else "none", 1, w_krsc.shape[1] // 2, 1, pre=True)
    M = ref.shape[0] * ref.shape[1] * ref.shape[2]
    ref, mag, pre = ref.reshape(M, -1), mag.reshape(M, -1), pre.reshape(M, -1)
    return _finish(name, mode, ref, mag, pre, relu, kred, [w_krsc.reshape(w_krsc.shape[0], -1)], [x4, w_krsc])


def _finish(name, mode, ref, mag, pre, relu, kred, weights, stored, hidden=(), frac_bits=0):
    if mode == "gauss":
        return ref, S.elem_bound(ref, mag, kred, "bf16")
    if mode == "round":
        return _round_preconditions(name, pre, relu), None
    S.prove_exact(name, ref, mag, weights, stored=stored, hidden=hidden, frac_bits=frac_bits)
    _both_sides(name, pre, relu)
    return ref, None


def _seed(*parts):
    s = 0
    for p in parts:
        for ch in str(p):
            s = (s * 131 + ord(ch)) % (1 << 31)
    return s


# ================================================================================================ mv_conv3x3_slice_fwd
MAPS = [(1, 1, 3), (1, 5, 2), (5, 1, 2), (2, 2, 40), (8, 16, 1), (3, 43, 1), (6, 9, 3), (2, 300, 1)]
# (H, W, B, S, N, pad behind S, cy, ldy); N % 32 == 16 leaves 16 sentinel columns behind the slice
SLICE_CASES = [(1, 1, 3, 16, 16, 16, 16, 64), (1, 5, 2, 48, 32, 0, 0, 32), (5, 1, 2, 16, 48, 16, 32, 112), (2, 2, 40, 48, 80, 16, 16, 128),
               (8, 16, 1, 128, 96, 0, 0, 96), (3, 43, 1, 16, 144, 16, 48, 224), (6, 9, 3, 128, 16, 16, 32, 80),
               (2, 300, 1, 16, 32, 0, 16, 64)]
SLICE_EDGE = (2, 13, 1, 512, 16, 16, 16, 64)         # the largest LDS mv_conv3x3_slice_supported admits: bound only (kred = 4608)
SLICE_ROUND = (6, 9, 3, 16, 32, 16, 16, 64)
SLICE_FLAGS = {"dense3x3_m64": "conv3x3_slice_m64", "dense3x3_m128": "conv3x3_slice_m128"}
assert flat_lds_bytes(128, 13, 512) <= FLAT_LDS_MAX < flat_lds_bytes(128, 14, 512)


def case_id(case):
    return "_".join("x".join(str(int(u)) for u in v) if isinstance(v, tuple) else str(int(v)) for v in case)


@functools.lru_cache(maxsize=None)
def slice_data(case, mode):
    H, W, B, S_, N, pad, cy, ldy = case
    rng = S.rng_of(_seed("slice", case, mode))
    x = _acts(rng, mode, (B, H, W, S_))
    wk, _ = _weights(rng, mode, N, 9 * S_, 4 * S_, 120, False)
    w = wk.reshape(N, 3, 3, S_)
    ref, bound = _finish3x3(f"slice/{case_id(case)}", mode, x, w, None, None, False, 9 * S_)
    M = B * H * W
    return {"kernel": "slice", "t": _rows_with_pad(x, pad).reshape(M, S_ + pad), "frag": pack3x3(w), "w": w, "S": S_, "N": N, "H": H, "W": W,
            "B": B, "cy": cy, "dests": [(M, ldy)], "slices": [(0, cy, ref, bound)], "kred": [9 * S_]}


def emu_slice(d, defect=None, arg=None):
    acc = flat_acc(d["t"], 0, d["S"], d["frag"], d["H"], d["W"], 9, _flat(defect), arg)
    (M, ld), N = d["dests"][0], d["N"]
    buf = new_dest(M, ld)
    put(buf, ld, d["cy"], store_bf(acc[:, :N], _store_mode(defect)))
    if defect == "upper_half_stored" and N % 32 == 16:
        put(buf, ld, d["cy"] + N, store_bf(acc[:, N:N + 16]))
    return [buf]


# ================================================================================================ mv_conv3x3_pair_fwd
# (H, W, B, (S0, S1), (N0, N1), (ct0, ct1), ldt, (cy0, cy1), ldy): channels of t that neither slice owns are NaN
_PA = ((16, 48), (16, 16), (64, 0), 96, (0, 48), 96)              # ct1 < ct0
_PB = ((48, 16), (80, 48), (0, 64), 80, (80, 0), 176)             # cy1 < cy0
_PC = ((128, 16), (96, 144), (16, 0), 160, (0, 112), 272)         # odd tile counts: 3 and 5
_PD = ((16, 16), (16, 16), (0, 32), 48, (32, 0), 64)
PAIR_CASES = [(1, 1, 3) + _PA, (1, 5, 2) + _PA, (5, 1, 2) + _PB, (2, 2, 40) + _PB, (8, 16, 1) + _PB, (3, 43, 1) + _PC, (6, 9, 3) + _PA,
              (2, 300, 1) + _PD]
PAIR_ROUND = (6, 9, 3) + _PD


@functools.lru_cache(maxsize=None)
def pair_data(case, mode):
    H, W, B, SS, NN, ct, ldt, cy, ldy = case
    rng = S.rng_of(_seed("pair", case, mode))
    M = B * H * W
    t = np.full((B, H, W, ldt), np.nan, F32)
    d = {"kernel": "pair", "H": H, "W": W, "B": B, "S": SS, "N": NN, "ct": ct, "cy": cy, "ldt": ldt, "dests": [(M, ldy)], "slices": [],
         "kred": [], "frag": [], "scale": [], "shift": [], "w": []}
    for i in range(2):
        x = _acts(rng, mode, (B, H, W, SS[i]))
        wk, sign = _weights(rng, mode, NN[i], 9 * SS[i], 4 * SS[i], 60, True)
        sc, sh = _scale_shift(rng, mode, NN[i])
        if mode == "round":
            wk[:, 4 * SS[i]] *= sc                                   # the carrier times the scale keeps its sign
        w = wk.reshape(NN[i], 3, 3, SS[i])
        ref, bound = _finish3x3(f"pair/{case_id(case)}/{i}", mode, x, w, sc, sh, True, 9 * SS[i])
        t[..., ct[i]:ct[i] + SS[i]] = x
        d["slices"].append((0, cy[i], ref, bound))
        d["kred"].append(9 * SS[i])
        d["frag"].append(pack3x3(w)), d["scale"].append(sc), d["shift"].append(sh), d["w"].append(w)
    d["t"] = t.reshape(M, ldt)
    return d


def emu_pair(d, defect=None, arg=None):
    M, ld = d["dests"][0]
    buf = new_dest(M, ld)
    for i in range(2):
        S_, N, ct = d["S"][i], d["N"][i], d["ct"][i]
        t2 = d["t"]
        if defect == "pair_uses_S0_pitch" and i == 1:
            ct = d["ct"][0]
            if ct + S_ > t2.shape[1]:
                t2 = np.concatenate([t2, np.full((M, ct + S_ - t2.shape[1]), np.nan, F32)], 1)
        acc = flat_acc(t2, ct, S_, d["frag"][i], d["H"], d["W"], 9, _flat(defect), arg)
        out = epi_relu(acc, d["scale"][i], d["shift"][i], defect)
        put(buf, ld, d["cy"][i], out[:, :N])
        if defect == "upper_half_stored" and N % 32 == 16:
            put(buf, ld, d["cy"][i] + N, out[:, N:N + 16])
    return [buf]


# ================================================================================================ mv_fire_expand_fwd
# (H, W, B, S, E, b1 null, b3 null)
FIRE_CASES = [(1, 1, 3, 16, 64, False, False), (1, 5, 2, 32, 64, True, False), (5, 1, 2, 48, 64, False, True), (2, 2, 40, 64, 256, False, False),
              (8, 16, 1, 16, 256, False, True), (3, 43, 1, 32, 64, True, False), (6, 9, 3, 48, 256, False, False),
              (2, 300, 1, 16, 64, False, False)]
FIRE_ROUND = (6, 9, 3, 16, 64, False, False)
FIRE_FALLBACK = (2, 300, 1, 64, 64, False, False)     # with "fire_expand_m256": the 256-pixel tile would need more than 64 KB
FIRE_FLAGS = {"": "fire_expand_m128", "fire_expand_m256": "fire_expand_m256"}
assert flat_lds_bytes(256, 300, 64) > FIRE_LDS_TWO >= flat_lds_bytes(256, 300, 16) and flat_lds_bytes(128, 300, 64) <= FLAT_LDS_MAX


@functools.lru_cache(maxsize=None)
def fire_data(case, mode):
    H, W, B, S_, E, n1, n3 = case
    rng = S.rng_of(_seed("fire", case, mode))
    M = B * H * W
    x = _acts(rng, mode, (B, H, W, S_))
    w1k, _ = _weights(rng, mode, E, S_, 0, 60, True)
    w3k, _ = _weights(rng, mode, E, 9 * S_, 4 * S_, 60, True)
    w1, w3 = w1k.reshape(E, 1, 1, S_), w3k.reshape(E, 3, 3, S_)
    b1 = None if n1 else _scale_shift(rng, mode, E)[1]
    b3 = None if n3 else _scale_shift(rng, mode, E)[1]
    r1, q1 = _finish3x3(f"fire/{case_id(case)}/1x1", mode, x, w1, None, b1, True, S_)
    r3, q3 = _finish3x3(f"fire/{case_id(case)}/3x3", mode, x, w3, None, b3, True, 9 * S_)
    tr = lambda w: np.ascontiguousarray(w.transpose(0, 3, 1, 2))
    return {"kernel": "fire", "t": x.reshape(M, S_), "f1": ops.fire_fragments(tr(w1)), "f3": ops.fire_fragments(tr(w3)), "b1": b1, "b3": b3,
            "w1": w1, "w3": w3, "S": S_, "E": E, "H": H, "W": W, "B": B, "dests": [(M, 2 * E)], "slices": [(0, 0, r1, q1), (0, E, r3, q3)],
            "kred": [S_, 9 * S_]}


def emu_fire(d, defect=None, arg=None):
    M, ld = d["dests"][0]
    E = d["E"]
    a1 = flat_acc(d["t"], 0, d["S"], d["f1"], d["H"], d["W"], 1)
    a3 = flat_acc(d["t"], 0, d["S"], d["f3"], d["H"], d["W"], 9, _flat(defect), arg)
    b1, b3 = d["b1"], d["b3"]
    if defect == "bias_of_other_half":
        b1, b3 = b3, b1
    if defect == "null_bias_reads_b1" and b3 is None:
        b3 = b1
    buf = new_dest(M, ld)
    for acc, b, c in ((a1, b1, 0), (a3, b3, E)):
        bv = np.zeros(E, F32) if b is None else np.roll(b, -16) if defect == "shift_from" else b
        put(buf, ld, c, store_bf(np.maximum(acc + bv, F32(0)), _store_mode(defect)))
    return [buf]


# ================================================================================================ pw128.h
def pw_acc(a, w, C, defect=None):
    """pw128_product: 64-channel chunks, min(4, channels left / 16) k-steps each, fp32."""
    a, w = np.asarray(a, F32), np.asarray(w, F32)
    nch = -(-C // 64)
    acc = np.zeros((a.shape[0], w.shape[0]), F32)
    for ch in range(nch):
        if defect == "drop_last_partial_chunk" and ch == nch - 1 and C % 64:
            continue
        src = ch - 2 if defect == "stale_buffer" and ch >= 2 else ch
        nks = 4 if defect == "read_past_C" else min((C - ch * 64) >> 4, 4)
        for ks in range(nks):
            k0 = src * 64 + ks * 16
            acc = acc + a[:, k0:k0 + 16] @ w[:, k0:k0 + 16].T
    return acc


def pw_put(bufs, dests, out, N, n0, c0, c1, defect=None):
    """pw128_epilogue with the split rule: group n < n0 -> dst0 column c0 + n, else dst1 column c1 + n - n0."""
    def where(n):
        if n < n0 or (defect == "n0_group_to_dst0" and n == n0) or len(bufs) == 1:
            return 0, c0 + n
        return 1, c1 + n - n0
    for n in range(0, N, 16):
        j, c = where(n)
        put(bufs[j], dests[j][1], c, out[:, n:n + 16])
    if defect == "dead_wave_stores":
        for n in range(N, -(-N // 128) * 128, 16):
            if (n // 64) * 64 >= N:                                  # the wave's first column is past N
                j, c = where(n)
                put(bufs[j], dests[j][1], c, np.zeros((out.shape[0], 16), F32))


# (M, C, N, n0, c0, ld0, c1, ld1); n0 == N: one destination
SPLIT_CASES = [(1, 16, 16, 16, 16, 96, 0, 0), (129, 64, 48, 16, 0, 32, 16, 64), (257, 80, 144, 48, 16, 80, 32, 144),
               (129, 128, 272, 128, 0, 144, 16, 176), (1, 144, 272, 256, 16, 288, 0, 32), (257, 144, 144, 144, 16, 176, 0, 0)]
SPLIT_ROUND = (129, 80, 48, 16, 0, 32, 16, 64)


@functools.lru_cache(maxsize=None)
def split_data(case, mode):
    M, C, N, n0, c0, ld0, c1, ld1 = case
    rng = S.rng_of(_seed("split", case, mode))
    x = _acts(rng, mode, (M, C))
    w, sign = _weights(rng, mode, N, C, 0, 60, True)
    sc, sh = _scale_shift(rng, mode, N)
    if mode == "round":
        w[:, 0] *= sc
    ref, mag, pre = S.gemm_ref(x, w, sc, sh, None, "relu", pre=True)
    ref, bound = _finish(f"split/{case_id(case)}", mode, ref, mag, pre, True, C, [w], [x, w])
    dests = [(M, ld0)] + ([(M, ld1)] if n0 < N else [])
    slices = [(0, c0, ref[:, :n0], None if bound is None else bound[:, :n0])]
    if n0 < N:
        slices.append((1, c1, ref[:, n0:], None if bound is None else bound[:, n0:]))
    return {"kernel": "split", "x": x, "w": w, "scale": sc, "shift": sh, "M": M, "C": C, "N": N, "n0": n0, "c0": c0, "c1": c1, "dests": dests,
            "slices": slices, "kred": [C] * len(slices)}


def emu_split(d, defect=None, arg=None):
    acc = pw_acc(d["x"], d["w"], d["C"], defect)
    out = epi_relu(acc, d["scale"], d["shift"], defect)
    bufs = [new_dest(M, ld) for M, ld in d["dests"]]
    pw_put(bufs, d["dests"], out, d["N"], d["n0"], d["c0"], d["c1"], defect)
    return bufs


# ================================================================================================ mv_preact_conv1x1_fwd
# (H, W, B, pool, C, N, post (s2 / h2) or identity, pad behind C, cy, ldy)
PREACT_CASES = [(1, 1, 1, 1, 16, 16, True, 16, 0, 16), (3, 43, 1, 1, 64, 48, True, 16, 0, 48), (1, 257, 1, 1, 80, 144, False, 16, 16, 176),
                (3, 43, 1, 1, 128, 272, True, 0, 0, 272), (1, 257, 1, 1, 144, 144, True, 16, 0, 144), (3, 43, 1, 1, 144, 16, False, 16, 32, 128),
                (2, 2, 1, 2, 16, 16, False, 16, 16, 48), (3, 2, 2, 2, 80, 48, True, 16, 0, 48), (2, 3, 2, 2, 64, 144, False, 16, 16, 176),
                (5, 7, 2, 2, 144, 272, True, 16, 0, 272), (15, 14, 2, 2, 128, 48, False, 16, 32, 96), (15, 14, 2, 2, 144, 144, True, 16, 0, 144)]
PREACT_ROUND = (6, 8, 2, 2, 80, 48, False, 16, 16, 80)
PREACT_MEAN = (4, 6, 2, 2, 16, 48, False, 16, 16, 80)
N_A = {1: 1, 2: 4}            # fp32 roundings of `a` in front of its bf16 rounding (module docstring)


def preact_kernel(case):
    return "preact1x1" + ("_pool2" if case[3] == 2 else "") + ("_relu" if case[6] else "")


def _pool64(r, pool):
    """(B, H, W, C) -> (B Ho Wo, C): the mean over the 2 x 2 windows, an odd last row / column dropped."""
    B, H, W, C = r.shape
    if pool == 2:
        Ho, Wo = H // 2, W // 2
        r = r[:, :2 * Ho, :2 * Wo].reshape(B, Ho, 2, Wo, 2, C).mean((2, 4))
    return r.reshape(-1, C)


def _preact_pad(x, pad):
    xp = _rows_with_pad(x, pad)
    if pad:
        xp[..., x.shape[-1] + 8:] = POISON
    return xp


@functools.lru_cache(maxsize=None)
def preact_data(case, mode):
    H, W, B, pool, C, N, post, pad, cy, ldy = case
    rng = S.rng_of(_seed("preact", case, mode))
    name = f"preact/{case_id(case)}"
    small = pool == 2 and mode == "int"               # quarter-integers: 4 |v| <= 256
    if mode == "round":                               # constant 2 x 2 windows: the means are the integers themselves
        assert pool == 2 and H % 2 == 0 and W % 2 == 0
        x = np.repeat(np.repeat(_acts(rng, mode, (B, H // 2, W // 2, C)), 2, 1), 2, 2)
    else:
        x = _acts(rng, mode, (B, H, W, C))
    if mode == "gauss":
        s1, h1 = _scale_shift(rng, mode, C)
    else:
        s1 = S.int_scale(rng, C, (1,) if small or mode == "round" else (1, 2))
        h1 = S.int_tensor(rng, (C,), 1 if small or mode == "round" else 2)
        if mode == "round":
            s1[0], h1[0] = 1.0, 0.0                   # the carrier channel: a = x in 9 .. 14
    w, sign = _weights(rng, mode, N, C, 0, 20, post)
    s2 = h2 = None
    if post:
        s2, h2 = _scale_shift(rng, mode, N)
        if small:
            s2, h2 = S.int_scale(rng, N, (1,)), S.int_tensor(rng, (N,), 4)
    x64 = x.astype(F64)
    r = np.maximum(x64 * s1.astype(F64) + h1.astype(F64), 0.0)
    a, mag_a = _pool64(r, pool), _pool64(np.abs(x64 * s1.astype(F64)) + np.abs(h1.astype(F64)), pool)
    aw = np.abs(w.astype(F64))
    if mode == "gauss":
        ea = N_A[pool] * 2.0 ** -23 * mag_a
        ea = ea + S.half_ulp_out(np.abs(a) + ea, "bf16")
        v, E, mag = a @ w.astype(F64).T, ea @ aw.T, (np.abs(a) + ea) @ aw.T
        if post:
            ref, mag, E = np.maximum(v * s2 + h2, 0.0), mag * np.abs(s2) + np.abs(h2), E * np.abs(s2)
        else:
            ref = v
        e_pre = E + (C + 4) * 2.0 ** -23 * mag
        bound = e_pre + S.half_ulp_out(np.abs(ref) + e_pre, "bf16")
    else:
        ref, mag, pre = S.epilogue64(a @ w.astype(F64).T, np.abs(a) @ aw.T, s2, h2, None, "relu" if post else "none", pre=True)
        assert (s1 < 0).any() and (r > 0).any() and ((x64 * s1 + h1) < 0).any(), f"{name}: the ReLU in front is not exercised"
        ref, bound = _finish(name, mode, ref, mag, pre, post, C, [w], [x, w], hidden=[a], frac_bits=2 if small else 0)
    Mo = a.shape[0]
    return {"kernel": "preact", "x": _preact_pad(x, pad), "w": w, "s1": s1, "h1": h1, "s2": s2, "h2": h2, "C": C, "N": N, "pool": pool, "H": H,
            "W": W, "B": B, "cy": cy, "a": a, "dests": [(Mo, ldy)], "slices": [(0, cy, ref, bound)], "kred": [C]}


@functools.lru_cache(maxsize=None)
def preact_mean_case():
    """The case for `round_before_mean` (module docstring): x = 2 k + 1 in [128, 255], s1 = +-2 (x takes its sign), h1 = 1, so the four
    relu(fma) of a window are 4 k + 3 in [259, 511] with sum(k) = 3 mod 4: their mean is = 2 mod 4 -- a bf16 value -- while
    each of them rounds UP to a multiple of 4, which moves the mean by 1 onto a tie that rounds away.  One +-1 weight per output."""
    H, W, B, pool, C, N, post, pad, cy, ldy = PREACT_MEAN
    rng = S.rng_of(_seed("preact-mean"))
    k = rng.integers(64, 124, (B, H // 2, 2, W // 2, 2, C))          # (b, ho, i, wo, j, c) is (b, 2 ho + i, 2 wo + j, c) in memory
    k[:, :, 1, :, 1] += (3 - k.sum((2, 4))) % 4
    r = (4 * k + 3).reshape(B, H, W, C)
    s1 = 2.0 * np.where(np.arange(C) % 3 == 0, -1.0, 1.0).astype(F32)
    h1 = np.ones(C, F32)
    x = ((r - 1) / 2 * np.sign(s1)).astype(F32)
    assert np.array_equal(S.bf(x), x) and r.max() <= 511 and r.min() >= 257
    a = _pool64(r.astype(F64), 2)
    assert np.array_equal(a % 4, np.full(a.shape, 2.0)) and np.array_equal(S.bf(a).astype(F64), a)
    w = np.zeros((N, C), F32)
    w[np.arange(N), np.arange(N) % C] = np.where(np.arange(N) % 2, -1.0, 1.0)
    ref = a @ w.astype(F64).T
    return {"kernel": "preact", "x": _preact_pad(x, pad), "w": w, "s1": s1, "h1": h1, "s2": None, "h2": None, "C": C, "N": N, "pool": 2, "H": H,
            "W": W, "B": B, "cy": cy, "a": a, "dests": [(a.shape[0], ldy)], "slices": [(0, cy, ref, None)], "kred": [C]}


def emu_preact(d, defect=None, arg=None, poison_nan_only=False):
    x = np.array(d["x"], F32)
    B, H, W, ldx = x.shape
    C, pool = d["C"], d["pool"]
    w, s1, h1 = d["w"], d["s1"], d["h1"]
    Cr = C
    if defect == "read_past_C":                       # all three masks lost: C rounded up to the chunk, the next row's weights
        Cr = min(-(-C // 64) * 64, ldx)
        if poison_nan_only:
            x[..., C:] = np.nan
        s1, h1 = np.concatenate([s1, np.ones(Cr - C, F32)]), np.concatenate([h1, np.zeros(Cr - C, F32)])
        flat = np.concatenate([w.reshape(-1), np.ones(Cr, F32)])
        w = flat[np.arange(w.shape[0])[:, None] * C + np.arange(Cr)[None, :]]
    if defect == "s1_abs":
        s1 = np.abs(s1)
    Ho, Wo = H // pool, W // pool
    pitch = 2 * Wo if defect == "pool_pitch_2Wo" and pool == 2 else W
    flat_x = x.reshape(-1, ldx)
    b, ho, wo = np.meshgrid(np.arange(B), np.arange(Ho), np.arange(Wo), indexing="ij")
    src = ((b * H + pool * ho) * pitch + pool * wo).reshape(-1)
    a = np.zeros((src.size, Cr), F32)
    with np.errstate(invalid="ignore"):
        for e in range(pool * pool):
            v = _fma(flat_x[np.minimum(src + (e >> 1) * pitch + (e & 1), flat_x.shape[0] - 1), :Cr], s1, h1)
            if defect != "relu_dropped_in_front":
                v = np.fmax(v, F32(0))                # fmaxf: a NaN operand gives the other one
            if defect == "round_before_mean":
                v = S.bf(v)
            a = a + v
        if pool == 2:
            a = a * F32(0.25)
        a = S.bf(a)
        if Cr % 16:
            a = np.concatenate([a, np.zeros((a.shape[0], 16 - Cr % 16), F32)], 1)
            w = np.concatenate([w, np.zeros((w.shape[0], 16 - Cr % 16), F32)], 1)
        acc = pw_acc(a, w, C, defect)
    out = epi_relu(acc, d["s2"], d["h2"], defect) if d["s2"] is not None else store_bf(acc, _store_mode(defect))
    bufs = [new_dest(M, ld) for M, ld in d["dests"]]
    pw_put(bufs, d["dests"], out, d["N"], d["N"], d["cy"], 0, defect)
    return bufs


# ================================================================================================ tables
DATA = {"slice": slice_data, "pair": pair_data, "fire": fire_data, "split": split_data, "preact": preact_data}
EMU = {"slice": emu_slice, "pair": emu_pair, "fire": emu_fire, "split": emu_split, "preact": emu_preact}
CASES = {"slice": SLICE_CASES, "pair": PAIR_CASES, "fire": FIRE_CASES, "split": SPLIT_CASES, "preact": PREACT_CASES}
ROUND = {"slice": SLICE_ROUND, "pair": PAIR_ROUND, "fire": FIRE_ROUND, "split": SPLIT_ROUND, "preact": PREACT_ROUND}

# every defect the instruments have to see: defect -> [(kernel, index into CASES[kernel], arg)]; "round" cases are added by the host
# module for the store defects.  The shapes are those at which the defect CAN show (module docstring).
REJECTED_AT = {
    "neighbour_image": [("slice", 0, None), ("slice", 1, None), ("slice", 2, None), ("slice", 3, None), ("pair", 6, None), ("fire", 3, None)],
    "row_wrap": [("slice", 2, None), ("slice", 4, None), ("slice", 5, None), ("pair", 5, None), ("fire", 7, None)],
    "swap_rs": [("slice", 1, None), ("slice", 2, None), ("slice", 6, None), ("pair", 3, None), ("fire", 6, None)],
    "drop_kstep": [("slice", 0, (4, 0)), ("slice", 4, (0, 7)), ("slice", 3, (8, 2)), ("pair", 5, (4, 0)), ("fire", 3, (2, 3))],
    "last_prefetch_repeat": [("slice", 2, None), ("slice", 3, None), ("slice", 4, None), ("pair", 5, None), ("fire", 4, None), ("fire", 6, None)],
    "upper_half_stored": [("slice", 0, None), ("slice", 2, None), ("slice", 3, None), ("slice", 5, None), ("pair", 0, None), ("pair", 3, None)],
    "second_tile_of_odd_count": [("slice", 0, None), ("slice", 1, None), ("slice", 3, None), ("slice", 4, None), ("slice", 5, None),
                                 ("pair", 5, None)],
    "pair_uses_S0_pitch": [("pair", i, None) for i in range(len(PAIR_CASES))],
    "shift_from": [("pair", 3, None), ("pair", 5, None), ("split", 1, None), ("split", 3, None), ("preact", 1, None), ("fire", 0, None)],
    "relu_before_affine": [("pair", 0, None), ("pair", 5, None), ("split", 0, None), ("split", 3, None), ("preact", 0, None), ("preact", 9, None)],
    "bias_of_other_half": [("fire", 0, None), ("fire", 1, None), ("fire", 2, None), ("fire", 6, None)],
    "null_bias_reads_b1": [("fire", 2, None), ("fire", 4, None)],
    "drop_last_partial_chunk": [("split", 0, None), ("split", 2, None), ("split", 4, None), ("preact", 0, None), ("preact", 7, None)],
    "stale_buffer": [("split", 4, None), ("split", 5, None), ("preact", 4, None), ("preact", 9, None)],
    "dead_wave_stores": [("split", 0, None), ("split", 1, None), ("split", 2, None), ("preact", 5, None), ("preact", 6, None)],
    "n0_group_to_dst0": [("split", 1, None), ("split", 2, None), ("split", 3, None), ("split", 4, None)],
    "pool_pitch_2Wo": [("preact", 8, None), ("preact", 9, None)],
    "relu_dropped_in_front": [("preact", i, None) for i in range(len(PREACT_CASES))],
    "s1_abs": [("preact", i, None) for i in range(len(PREACT_CASES))],
    "read_past_C": [("preact", 0, None), ("preact", 2, None), ("preact", 7, None)],
}
STORE_DEFECTS = ("trunc", "half_up")                   # rejected by mode "round" at every kernel; trunc also by the bias rule
SPECIAL = {"round_before_mean": "preact_mean_case"}
NOT_REJECTED = {"halo_not_zero_past_M": "an out-of-bounds read, never a wrong value: no live tap reaches a slot past M (module docstring)"}
ISSUE_DEFECTS = ("neighbour_image", "row_wrap", "halo_not_zero_past_M", "swap_rs", "drop_kstep", "last_prefetch_repeat", "upper_half_stored",
                 "second_tile_of_odd_count", "pair_uses_S0_pitch", "trunc", "shift_from", "relu_before_affine", "bias_of_other_half",
                 "null_bias_reads_b1", "drop_last_partial_chunk", "stale_buffer", "dead_wave_stores", "n0_group_to_dst0", "round_before_mean",
                 "pool_pitch_2Wo", "relu_dropped_in_front", "s1_abs", "read_past_C")
