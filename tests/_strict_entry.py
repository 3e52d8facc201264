"""Strict instruments for the kernels on the ENTRY path into the GEMM cores (CPU only; GPU side: tests/test_strict_entry_gpu.py,
proofs: tests/test_strict_entry_host.py): the fp32-input image entries (mv_conv2d_nchw_fwd, mv_conv2d_nchw_f32out_fwd,
mv_conv2d_nchw_split_fwd, mv_stem_conv_pool_fwd), the generic NCHW fallback in token mode, mv_linear_split_fwd, the head-major stores
of mv_linear_heads_fwd / mv_linear_lnin_fwd, and mv_vit_cls_pos_fwd.  The two instruments are those of tests/_strict.py (exact
operands -> equality; Gaussian operands -> elem_bound on every element + the rounding-bias rule).  New here:

A. Rounding-visible images (`visible_image`).  Every strict image so far was a bf16 value already, so the kernels' fp32 -> bf16
   operand rounding was a no-op.  Here every pixel is 32 + q/4 + f, q in {0..3}, f in {1/8, 1/8 + 2^-12, 1/8 - 2^-12, 0} drawn with
   probabilities (0.4, 0.3, 0.2, 0.1).  bf16 spacing in [32, 64) is 1/4: f = 1/8 is an exact tie (to q for even q, to q + 1 for odd q),
   the next two round up / down past the tie, and the RNE image is a multiple of 1/4.  Truncation differs from RNE wherever RNE rounds
   up (~50 % of the pixels), round-half-up wherever a tie sits above an even value (~20 %).  Weight rows hold as many +1 as -1
   (`balanced_rows`: 2 + 2, or 3 + 3 where 4 per row cannot cover the reduction -- the issue's 2 + 2 cannot at K = 32, C R S = 147),
   scale 1, integer shifts.  Products are exact, every partial sum is a multiple of 1/4 far below 2^22 (exact in fp32 in any order).
   The issue's claim |out| <= 3 + |shift| holds only where the whole window is inside the image: with padding a border window can
   keep up to three taps of one sign (~101), and between 64 and 128 only multiples of 1/2 are bf16 values.  The construction is
   therefore amended: inside a band of R pixels along the border a pixel whose RNE value is an odd multiple of 1/4 gets q ^ 1 (its
   RNE value becomes even; its kind -- tie / above / below -- is kept).  `prove_visible` does not rely on that argument: it asserts
   directly that every reference output (and the conv map under the pool) IS a bf16 value, the accumulator limit, the coverage, and
   the tie / truncation / half-up fractions.  The reference is taken on the RNE image and the result must EQUAL it.
   mv_patch4_ln_fwd is not repeated here: tests/_strict_lngemm.py: patch4_gauss already feeds un-rounded fp32 pixels (rng.random)
   against a reference on the RNE image, and tests/test_strict_lngemm_host.py::test_patch4_ln_bound shows its `trunc_pack` defect
   (the image truncated) outside the bound on every case.  mv_stem_conv_pool_fwd's images (tests/test_strict_gpu.py) were bf16
   values: it is run here.

B. Split weights w = a + b 2^-10 (a in [-2, 2], b in [-3, 3] integers): hi = bf16(w), lo = bf16(w - hi), hi + lo == w exactly
   (asserted; hi == a except at |a| = 1 with b = -3 sign(a), where hi = +-255/256 and lo = -+2^-10).  With integer x in [-4, 4] every
   product and partial sum is a multiple of 2^-10 below 2^13: exact in fp32 in any order, as are the integer scale, shift and
   residual (`prove_dyadic`).  An fp32 output must EQUAL the float64 reference; a bf16 output (mv_conv2d_nchw_split_fwd has no other)
   is ONE rounding of that exact value and must EQUAL bf16_rne(ref) -- the issue's "single output rounding" with nothing left over.
   Gaussian: the reference is float64 on hi + lo; K_red counts both planes (2 C R S, 2 K).

C. Head-major stores: integer operands per prove_exact plus a shift that encodes the column, 16 (n / 64) + n % 16 - 48, so that a
   swapped head or q / k / v group changes values; the whole [B][3H][tokens][dh] buffer is compared.

Emulations (float32, numpy) with one defect switch each, and where each defect is rejected (tests/test_strict_entry_host.py):
    truncate_x, half_up_x     image operand truncated / rounded half-up          visible-exact (A); invisible to every bf16-valued image
    truncate_store            bf16 store truncates                                bias rule; exact split-conv (single rounding)
    drop_lo                   second weight plane not accumulated                 exact, bound
    lo_k_shift                second plane read one k-tile late                   exact, bound
    lo_pad_garbage            pad columns of the second plane not zero            exact, bound at C R S = 27 (padded to 32)
    remainder_rows_read       patches taken from the last H - H % R rows          exact, bound at H = 70
    pos_off_by_one            tok_offset ignored for the position row             exact, bound
    cls_row_written           row 0 of each image written                         sentinel check
    token_major_store         [M][N] rows instead of head-major                   exact, bound
    image_index_per_tile      image index from the tile's first row               exact, bound at tokens = 197 and 50
    qkv_group_swap            k and v groups trade places                         exact, bound
Not rejected, with the reason:
    image_index_per_tile at tokens = 256: 256-row tiles never straddle an image there, the defect changes nothing (that case is the
        aligned control); lo_pad_garbage at C R S = 147 -> 160 is rejected too, but at a reduction that is a multiple of 16 there are
        no pad columns and it is the honest kernel; remainder_rows_read where H % R == 0 likewise.
"""
from __future__ import annotations

import functools

import numpy as np
import torch

from tests import _strict as S
from tests._strict import F32, F64, SENTINEL, bf, bf16_truncate, rng_of

U10 = 2.0 ** -10


def _ro(*arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)


# ================================================================================================ A. rounding-visible images
F_TABLE = np.array([0.125, 0.125 + 2.0 ** -12, 0.125 - 2.0 ** -12, 0.0])
F_PROB = (0.4, 0.3, 0.2, 0.1)


def bf16_half_up(a):
    """fp32 -> bf16 by adding half an ulp to the magnitude and truncating (the round-half-up mutant)."""
    a = np.ascontiguousarray(np.asarray(a, F32))
    return ((a.view(np.uint32) + np.uint32(0x8000)) & np.uint32(0xffff0000)).view(F32)


def is_tie(a):
    return (np.ascontiguousarray(np.asarray(a, F32)).view(np.uint32) & np.uint32(0xffff)) == np.uint32(0x8000)


def visible_image(seed, shape, band):
    """(N, C, H, W) fp32 pixels 32 + q/4 + f (module docstring); inside `band` pixels of the border the RNE value is a multiple of 1/2."""
    rng = rng_of(seed)
    q = rng.integers(0, 4, shape)
    fi = rng.choice(4, shape, p=F_PROB)
    r4 = q + (fi == 1) + ((fi == 0) & (q % 2 == 1))                      # 4 (RNE value - 32)
    H, W = shape[-2], shape[-1]
    hh, ww = np.arange(H)[:, None], np.arange(W)[None, :]
    inband = (hh < band) | (hh >= H - band) | (ww < band) | (ww >= W - band)
    q = np.where(inband & (r4 % 2 == 1), q ^ 1, q)
    x = (32.0 + q / 4.0 + F_TABLE[fi]).astype(F32)
    assert np.array_equal(x.astype(F64), 32.0 + q / 4.0 + F_TABLE[fi])
    return x


def balanced_rows(rng, rows, kred, half):
    """(rows, kred): every row holds exactly `half` +1 and `half` -1; every reduction index is used (S.pm1_rows' cyclic walk)."""
    nnz = 2 * half
    cover = -(-kred // rows)
    assert cover <= nnz <= kred, f"balanced_rows: {rows} rows x {nnz} cannot cover {kred}"
    perm = rng.permutation(kred)
    w = np.zeros((rows, kred), F32)
    for r in range(rows):
        pos = perm[(r * cover + np.arange(cover)) % kred]
        free = np.setdiff1d(np.arange(kred), pos)
        pos = np.concatenate([pos, rng.choice(free, nnz - cover, replace=False)])
        w[r, pos] = rng.permutation(np.repeat(np.array([1.0, -1.0], F32), half))
    return w


def pair_rows(rng, hi, taps):
    """The second plane of a rounding-visible split filter: per row one +1 and one -1 where `hi` is zero, at the SAME tap of two
    channels (k = c taps + t) -- a border window keeps both or neither, so the plane adds nothing to the unbalanced border sums."""
    lo = np.zeros_like(hi)
    for r in range(hi.shape[0]):
        free = [t for t in rng.permutation(taps) if hi[r, t] == 0 and hi[r, taps + t] == 0]
        lo[r, free[0]], lo[r, taps + free[0]] = 1.0, -1.0
    return lo


def visible_half(K, kred):
    """+1s (= -1s) per row: 2, or 3 where four non-zeros per row cannot cover the reduction."""
    return 2 if -(-kred // K) <= 4 else 3


def _conv64_nchw(x, w, stride, pad):
    y = torch.nn.functional.conv2d(torch.from_numpy(np.asarray(x, F64)), torch.from_numpy(np.asarray(w, F64)), None, stride, pad)
    return y.permute(0, 2, 3, 1).contiguous().numpy()                   # NHWC rows


def is_bf16(a):
    a = np.asarray(a, F64)
    return np.array_equal(bf(a.astype(F32)).astype(F64), a)


def prove_visible(name, x, weights, shift, ref, mag, hidden=(), out="bf16"):
    """Preconditions of the rounding-visible exact case, asserted on the CPU (module docstring, A)."""
    xr = bf(x).astype(F64)
    assert np.array_equal(np.rint(xr * 4), xr * 4) and np.abs(xr).max() < 64, f"{name}: RNE image not on the 1/4 lattice"
    for w in weights:
        assert np.isin(np.asarray(w), (-2.0, -1.0, 0.0, 1.0, 2.0)).all(), f"{name}: weights not small integers"
    assert np.array_equal(np.rint(np.asarray(shift, F64)), np.asarray(shift, F64)), f"{name}: shift not integer"
    assert np.abs(mag).max() * 4 < S.ACC_INT_MAX, f"{name}: accumulator limit"
    for what, a in [("ref", ref)] + [(f"hidden[{i}]", h) for i, h in enumerate(hidden)]:
        assert np.array_equal(np.rint(np.asarray(a, F64) * 4), np.asarray(a, F64) * 4), f"{name}: {what} off the 1/4 lattice"
        if out == "bf16" or what != "ref":
            assert is_bf16(a), f"{name}: {what} holds values that are no bf16 values"
    S._prove_coverage(name, [np.asarray(weights[0]).reshape(weights[0].shape[0], -1)])
    assert float((np.asarray(ref) == 0).mean()) < 0.9, f"{name}: the reference is mostly zero"
    f = visible_fractions(x)
    assert f["ties"] >= 0.25 and f["trunc_differs"] >= 0.25 and f["half_up_differs"] >= 0.10, f"{name}: {f}"
    return f


def visible_fractions(x):
    r = bf(x)
    return {"ties": float(is_tie(x).mean()), "trunc_differs": float((bf16_truncate(x) != r).mean()),
            "half_up_differs": float((bf16_half_up(x) != r).mean()), "non_bf16": float((r != x).mean())}


# ================================================================================================ NCHW entry cases
# (tag, N, H, W, K, R, stride, pad, tokens): the three epilogues of stem.hip (tests/test_strict_act_gpu.py: STEM_ACT_CASES)
STEM_GEOMS = [("3x3_s2_33x35_k24", 2, 33, 35, 24, 3, 2, 1, False), ("7x7_s2_61x75", 1, 61, 75, 32, 7, 2, 3, False),
              ("patch16_tokens_64x64", 2, 64, 64, 768, 16, 16, 0, True)]
STEM_KERNELS = {"3x3_s2_33x35_k24": "stem_conv_mfma", "7x7_s2_61x75": "stem_patch_mfma", "patch16_tokens_64x64": "patch_embed_mfma"}
# mv_conv2d_nchw_f32out_fwd: M = 32 and 30 rows per pair of images (one ragged 128-row tile); K = 200: a ragged second 128-channel
# tile; H = 70: six rows below the last patch row that no patch may read; tokens: row n T + 1 + p, the class row keeps the sentinel
F32OUT_GEOMS = [("64x64_k768_tok", 2, 64, 64, 768, 16, 16, 0, True), ("40x72_k200_dense", 2, 40, 72, 200, 16, 16, 0, False),
                ("70x64_k200_tok", 2, 70, 64, 200, 16, 16, 0, True)]
# (R, S, stride_h, stride_w, pad, flag) on 3 x 64 x 72 images, K = 200: what mv_conv2d_nchw_f32out_supported must refuse
F32OUT_REFUSALS = [("overlap", 16, 16, 8, 8, 0, None), ("padding", 16, 16, 16, 16, 1, None), ("s_mod_8", 16, 12, 16, 12, 0, None),
                   ("flag", 16, 16, 16, 16, 0, "no_patch_f32out")]
SPLIT_GEOMS = STEM_GEOMS[:2]              # C R S = 27 (padded to 32: the pad columns of BOTH planes) and 147 (to 160)
# mv_stem_conv_pool_fwd (tests/test_strict_gpu.py: test_stem_pool): (tag, N, H, W, R, stride, pad, pool pad, scale, kernel)
POOL_GEOMS = [("resnet_75x93", 2, 75, 93, 7, 2, 3, 1, True, "stem_pool_mfma_f32in"), ("alexnet_67x67", 2, 67, 67, 11, 4, 2, 0, False, "stem_pool11_mfma_f32in")]


def geom_id(g):
    return g[0]


def _odims(H, W, R, S_, sh, sw, pad):
    return (H + 2 * pad - R) // sh + 1, (W + 2 * pad - S_) // sw + 1


def split_weights(rng, shape):
    """w = a + b 2^-10 -> (w fp32, hi, lo) with hi + lo == w exactly."""
    a, b = rng.integers(-2, 3, shape), rng.integers(-3, 4, shape)
    w = (a + b * U10).astype(F32)
    hi = bf(w)
    lo = bf(w - hi)
    assert np.array_equal(hi.astype(F64) + lo.astype(F64), a + b * U10) and np.array_equal(bf(w - hi), w - hi)
    return w, hi, lo


def gauss_split(rng, shape, kred):
    w = (rng.standard_normal(shape) / np.sqrt(kred)).astype(F32)
    hi = bf(w)
    return w, hi, bf(w - hi)


def prove_dyadic(name, pre, mag, weights, min_lo=0.5):
    """B's preconditions: the pre-activation and its magnitude are multiples of 2^-10 below 2^24 2^-10 (S.prove_exact, fp32), the
    weights cover the reduction, and at least `min_lo` of the low plane is non-zero."""
    S.prove_exact(name, pre, mag, weights[:1], out="fp32", frac_bits=10)
    nz = float((np.asarray(weights[1]) != 0).mean())
    assert nz >= min_lo, f"{name}: only {100 * nz:.0f} % of the low plane is non-zero"
    return nz


@functools.lru_cache(maxsize=None)
def nchw_case(kind, mode, tag, N, H, W, K, R, stride, pad, tokens, xdtype, out, xbf=False, seed=71):
    """One launch of an NCHW entry.  kind: "plain" (mv_conv2d_nchw_fwd / _f32out_fwd / the generic fallback; one bf16 filter) or
    "split" (two planes).  mode: "int" / "gauss" (tests/_strict.py), "visible" (A; fp32 images only) or "dyadic" (B; split only).
    -> dict: x, hi, lo, scale, shift, pos, full (the whole destination [N][T or P][K] as it must look afterwards, sentinel rows
    included), ref / mag / kred (the written rows [N][P][K]), exact (compare for equality), T."""
    C, S_ = 3, R
    rng = rng_of(seed + (0 if mode in ("int", "visible", "dyadic") else 1))
    Ho, Wo = _odims(H, W, R, S_, stride, stride, pad)
    P, crs = Ho * Wo, C * R * S_
    # gauss: an fp32 image keeps its un-rounded pixels (the reference is taken on their RNE values) unless `xbf` (the generic fallback
    # multiplies fp32 pixels as they are: its images are bf16 values)
    q = bf if xdtype == "bf16" or xbf else (lambda a: np.asarray(a, F32))
    lo = None
    if mode == "visible":
        assert xdtype == "fp32"
        x = visible_image(seed, (N, C, H, W), R if pad else 0)
        hi = balanced_rows(rng, K, crs, visible_half(K, crs)).reshape(K, C, R, S_)
        if kind == "split":
            lo = pair_rows(rng, hi.reshape(K, crs), R * S_).reshape(K, C, R, S_)
        sc, sh = None, S.int_tensor(rng, (K,), 8)
    elif mode == "dyadic":
        x = S.int_tensor(rng, (N, C, H, W), 4)
        _, hi, lo = split_weights(rng, (K, C, R, S_))
        sc, sh = S.int_scale(rng, K), S.int_tensor(rng, (K,), 8)
    elif mode == "int":
        x = S.int_tensor(rng, (N, C, H, W), 2)
        hi = S.pm1_rows(rng, K, crs, 16).reshape(K, C, R, S_)
        sc, sh = S.int_scale(rng, K), S.int_tensor(rng, (K,), 8)
    else:
        x = q(rng.standard_normal((N, C, H, W)))
        if kind == "split":
            _, hi, lo = gauss_split(rng, (K, C, R, S_), crs)
        else:
            hi = bf(rng.standard_normal((K, C, R, S_)) / np.sqrt(crs))
        sc, sh = S.gauss_scale(rng, K), (0.1 * rng.standard_normal(K)).astype(F32)
    pos = res = None
    T = P + 1 if tokens else 0
    if tokens:
        pos = rng.standard_normal((T, K)).astype(F32) if mode == "gauss" else S.int_tensor(rng, (T, K), 4)
        res = np.broadcast_to(pos[1:].reshape(1, Ho, Wo, K), (N, Ho, Wo, K))
    xr = bf(x).astype(F64)                                                  # what the MFMA sees (fp32 images are rounded: header)
    weff = hi.astype(F64) + (0.0 if lo is None else lo.astype(F64))
    wabs = np.abs(hi).astype(F64) + (0.0 if lo is None else np.abs(lo).astype(F64))
    acc, amag = _conv64_nchw(xr, weff, stride, pad), _conv64_nchw(np.abs(xr), wabs, stride, pad)
    ref, mag = S.epilogue64(acc, amag, sc, sh, res, 0)
    kred = crs * (2 if kind == "split" else 1) + (1 if tokens else 0)
    info = {}
    if mode == "visible":
        info = prove_visible(f"{kind}/{tag}", x, [hi] + ([lo] if lo is not None else []), sh, ref, mag, out=out)
    elif mode == "dyadic":
        info = {"lo_nonzero": prove_dyadic(f"{kind}/{tag}", ref, mag, [hi.reshape(K, -1), lo.reshape(K, -1)])}
        assert np.abs(x).max() <= 4 and np.array_equal(np.rint(x), x)
        if out == "bf16":
            ref = bf(ref.astype(F32)).astype(F64)                           # exact in fp32 (proved above), then ONE rounding
    elif mode == "int":
        S.prove_exact(f"{kind}/{tag}", ref, mag, [hi], stored=[x, hi], out=out)
    ref, mag = ref.reshape(N, P, K), mag.reshape(N, P, K)
    full = ref
    if tokens:
        full = np.concatenate([np.full((N, 1, K), SENTINEL), ref], 1)
    d = dict(kind=kind, mode=mode, tag=tag, N=N, C=C, H=H, W=W, K=K, R=R, stride=stride, pad=pad, T=T, P=P, xdtype=xdtype, out=out,
             x=x, hi=hi, lo=lo, scale=sc, shift=sh, pos=pos, ref=ref, mag=mag, full=full, kred=kred, exact=mode != "gauss", info=info)
    _ro(x, hi, lo, sc, sh, pos, ref, mag, full)
    return d


@functools.lru_cache(maxsize=None)
def pool_case(tag, N, H, W, R, stride, pad, pp, with_scale, seed=72):
    """mv_stem_conv_pool_fwd on a rounding-visible image: conv + shift + ReLU + max-pool 3 / 2, everything on the 1/4 lattice and a
    bf16 value (so it does not matter whether the kernel rounds before or after the max)."""
    C, K = 3, 64
    rng = rng_of(seed)
    x = visible_image(seed, (N, C, H, W), R)
    w = balanced_rows(rng, K, C * R * R, visible_half(K, C * R * R)).reshape(K, C, R, R)
    sc = np.ones(K, F32) if with_scale else None
    sh = S.int_tensor(rng, (K,), 8)
    xr = bf(x).astype(F64)
    conv, cmag = S.epilogue64(_conv64_nchw(xr, w, stride, pad), _conv64_nchw(np.abs(xr), np.abs(w), stride, pad), sc, sh, None, 1)
    pool = lambda a: torch.nn.functional.max_pool2d(torch.from_numpy(a).permute(0, 3, 1, 2), 3, 2, pp).permute(0, 2, 3, 1).contiguous().numpy()
    ref, mag = pool(conv), pool(cmag)
    info = prove_visible(f"stem_pool/{tag}", x, [w], sh, ref, mag, hidden=[conv])
    _ro(x, w, sc, sh, ref, mag)
    return dict(x=x, w=w, scale=sc, shift=sh, ref=ref, mag=mag, info=info, pool=pool, stride=stride, pad=pad, R=R)


# ------------------------------------------------------------------------------------------------ emulation of the NCHW entries
NCHW_DEFECTS = ("truncate_x", "half_up_x", "truncate_store", "drop_lo", "lo_k_shift", "lo_pad_garbage", "remainder_rows_read",
                "pos_off_by_one", "cls_row_written")


def _im2col(x, R, S_, stride, pad):
    """[N][C][H][W] -> rows [N P][C R S] in the filter's OIHW order."""
    u = torch.nn.functional.unfold(torch.from_numpy(np.ascontiguousarray(x, dtype=F32)), (R, S_), padding=pad, stride=stride)
    return u.permute(0, 2, 1).reshape(-1, u.shape[1]).numpy()


def _gemm32(a, b, chunk=16):
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    acc = np.zeros((a.shape[0], b.shape[0]), F32)
    for k0 in range(0, a.shape[1], chunk):
        acc = acc + a[:, k0:k0 + chunk] @ b[:, k0:k0 + chunk].T
    return acc


def emu_nchw(d, defect=None, pooled=None):
    """The entry's contract in float32: the image rounded to bf16 (RNE), fp32 accumulation over hi then lo in 16-wide steps,
    * scale + shift + position row, the store; written into a sentinel-filled destination at row n T + 1 + p.  One defect each
    (module docstring).  `pooled`: a pool_case dict -- ReLU and the max-pool follow."""
    x = np.asarray(d["x"] if pooled is None else pooled["x"], F32)
    xr = bf16_truncate(x) if defect == "truncate_x" else (bf16_half_up(x) if defect == "half_up_x" else bf(x))
    if pooled is not None:
        R = pooled["R"]
        rows = _im2col(xr, R, R, pooled["stride"], pooled["pad"])
        w = np.asarray(pooled["w"], F32)
        v = _gemm32(rows, w.reshape(w.shape[0], -1)) * (F32(1) if pooled["scale"] is None else pooled["scale"]) + pooled["shift"]
        N, H, W = x.shape[0], x.shape[2], x.shape[3]
        Ho, Wo = _odims(H, W, R, R, pooled["stride"], pooled["stride"], pooled["pad"])
        y = pooled["pool"](np.maximum(v, 0).reshape(N, Ho, Wo, -1).astype(F64)).astype(F32)
        return bf16_truncate(y) if defect == "truncate_store" else bf(y)
    N, K, R, P, T, H = d["N"], d["K"], d["R"], d["P"], d["T"], d["H"]
    if defect == "remainder_rows_read" and d["stride"] == R and H % R:
        xr = xr[:, :, H % R:]
    rows = _im2col(xr, R, R, d["stride"], d["pad"])
    hi = np.asarray(d["hi"], F32).reshape(K, -1)
    acc = _gemm32(rows, hi)
    crs = hi.shape[1]
    if d["lo"] is not None and defect != "drop_lo":
        lo = np.asarray(d["lo"], F32).reshape(K, -1)
        if defect == "lo_k_shift":                                          # the plane read 16 columns late; behind it, the sentinel
            lo = np.concatenate([lo[:, 16:], np.full((K, 16), SENTINEL, F32)], 1)[:, :crs]
        acc = acc + _gemm32(rows, lo)
        if defect == "lo_pad_garbage" and crs % 16:                        # stale row data times a pad column that is not zero
            acc = acc + rows[:, :1] * F32(16 - crs % 16)
    v = acc if d["scale"] is None else acc * np.asarray(d["scale"], F32)
    v = (v + np.asarray(d["shift"], F32)).reshape(N, P, K)
    if T:
        off = 0 if defect == "pos_off_by_one" else 1
        v = v + np.asarray(d["pos"], F32)[None, off:off + P]
    y = np.asarray(v, F32) if d["out"] == "fp32" else (bf16_truncate(v) if defect == "truncate_store" else bf(v))
    if not T:
        return y
    full = np.full((N, T, K), SENTINEL, F32)
    full[:, 1:] = y
    if defect == "cls_row_written":
        full[:, 0] = 0.0
    return full


# ================================================================================================ C. mv_linear_split_fwd
def split_tile(M, N, K, min_nk=40):
    """route.h: route_linear_split -> (tile name, split-K engages with scratch on offer).  The rule of igemm8_wanted on the fused
    reduction 2 K, and the half-size tile by N where it declines."""
    nk = 2 * K // 64
    tm256, tm128, tn = -(-M // 256), -(-M // 128), -(-N // 256)
    t = 0
    if nk >= 4 and N >= 96:
        t = (3 if tm256 >= 90 else 0) if N <= 128 else (1 if tm256 * tn >= 150 else (2 if tm128 * tn >= 40 else 0))
    if t == 0:
        t = 3 if N <= 128 else 2
    tiles = tm128 * tn if t == 2 else tm256 * -(-N // 128)
    return {1: "256x256", 2: "128x256", 3: "256x128"}[t], (t != 1 and tiles <= 128 and nk >= min_nk)


# (tag, M, N, K): the smallest (M, N) per tile by the rule (256x128: N <= 128; 128x256: N > 128; 256x256: N > 128, K >= 128 and
# ceil(M / 256) ceil(N / 256) >= 150 -- 75 x 2 with one row / eight columns in the last tiles is the smallest M N), the issue's two
# ragged shapes, and both K at both half-size tiles.  K = 64: one k-tile per plane; 192: three (the lo plane starts at k-tile 3 of 6).
LSPLIT_SHAPES = [("t256x128_min", 1, 8, 64), ("t128x256_min", 1, 136, 64), ("t256x256_min", 74 * 256 + 1, 264, 192),
                 ("ragged_37x72", 37, 72, 64), ("ragged_300x136", 300, 136, 192), ("t256x128_k192", 260, 128, 192),
                 ("t128x256_k64", 130, 264, 64)]
LSPLIT_TILES = {"t256x128_min": "256x128", "t128x256_min": "128x256", "t256x256_min": "256x256", "ragged_37x72": "256x128",
                "ragged_300x136": "128x256", "t256x128_k192": "256x128", "t128x256_k64": "128x256"}
# (tag, scale, shift, residual, act)
LSPLIT_EPILOGUES = [("plain", False, False, False, 0), ("shift_relu", False, True, False, 1), ("scale_shift_res", True, True, True, 0),
                    ("scale_shift_res_relu", True, True, True, 1)]
LSPLIT_SPLITK = ("ragged_300x136", 300, 136, 192)          # 3 x 1 tiles of 128 x 256, six k-tiles: splits with splitk_min_nk = 6
LSPLIT_REFUSALS = [("k_mod_64", 64, 72, 96, "bf16", None), ("fp32_x", 64, 72, 64, "fp32", None), ("force_generic", 64, 72, 64, "bf16", "force_generic")]


@functools.lru_cache(maxsize=8)
def lsplit_case(mode, M, N, K, with_scale, with_shift, with_res, act, out, seed=73):
    rng = rng_of(seed + (0 if mode == "int" else 1))
    if mode == "int":
        x = S.int_tensor(rng, (M, K), 4)
        w, hi, lo = split_weights(rng, (N, K))
        sc = S.int_scale(rng, N) if with_scale else None
        sh = S.int_tensor(rng, (N,), 8) if with_shift else None
        res = S.int_tensor(rng, (M, N), 16) if with_res else None
    else:
        x = bf(rng.standard_normal((M, K)))
        w, hi, lo = gauss_split(rng, (N, K), K)
        sc = S.gauss_scale(rng, N) if with_scale else None
        sh = (0.1 * rng.standard_normal(N)).astype(F32) if with_shift else None
        res = (bf if out == "bf16" else (lambda a: np.asarray(a, F32)))(rng.standard_normal((M, N))) if with_res else None
    x64 = x.astype(F64)
    acc = x64 @ (hi.astype(F64) + lo.astype(F64)).T
    amag = np.abs(x64) @ (np.abs(hi).astype(F64) + np.abs(lo).astype(F64)).T
    ref, mag, pre = S.epilogue64(acc, amag, sc, sh, res, act, pre=True)
    info = {}
    if mode == "int":
        assert out == "fp32"
        info = {"lo_nonzero": prove_dyadic(f"lsplit/{M}x{N}x{K}", pre, mag, [hi, lo])}
    wcat = np.ascontiguousarray(np.concatenate([hi, lo], 1))                # [N][2K] = [w_hi row | w_lo row]
    _ro(x, hi, lo, wcat, sc, sh, res, ref, mag)
    return dict(x=x, hi=hi, lo=lo, wcat=wcat, scale=sc, shift=sh, res=res, act=act, ref=ref, mag=mag, kred=2 * K, out=out, info=info)


LSPLIT_DEFECTS = ("drop_lo", "lo_k_shift", "truncate_store")


def emu_lsplit(d, defect=None):
    """[x | x] . [w_hi | w_lo]^T in float32, 64-wide k-tiles, the epilogue, the store.  lo_k_shift: the second plane is read one
    k-tile (64 columns) late in the [N][2K] buffer -- the tail comes from the next row's hi plane (the sentinel behind the last)."""
    x, wcat = np.asarray(d["x"], F32), np.asarray(d["wcat"], F32)
    N, K = wcat.shape[0], wcat.shape[1] // 2
    hi, lo = wcat[:, :K], wcat[:, K:]
    if defect == "lo_k_shift":
        flat = np.concatenate([wcat.reshape(-1), np.full(64, SENTINEL, F32)])
        lo = flat[np.arange(N)[:, None] * 2 * K + K + 64 + np.arange(K)[None, :]]
    acc = _gemm32(x, hi, 64)
    if defect != "drop_lo":
        acc = acc + _gemm32(x, lo, 64)
    v = acc if d["scale"] is None else acc * np.asarray(d["scale"], F32)
    if d["shift"] is not None:
        v = v + np.asarray(d["shift"], F32)
    if d["res"] is not None:
        v = v + np.asarray(d["res"], F32)
    v = S.act32(v, S.act_name(d["act"]))
    return np.asarray(v, F32) if d["out"] == "fp32" else (bf16_truncate(v) if defect == "truncate_store" else bf(v))


# ================================================================================================ D. head-major stores
HEADS_K, HEADS_H, HEADS_DH = 256, 2, 64
HEADS_N = 3 * HEADS_H * HEADS_DH
HEADS_TOKENS = (197, 50, 256)             # 197, 50: image boundaries inside 256-row tiles; 256: aligned


def heads_batch(tokens):
    """The smallest B with B tokens >= 4096 (route.h: igemm2_wanted, the entry's gate)."""
    return -(-4096 // tokens)


# flags -> kernel (route.h: route_linear_heads; with_scale decides lin / dense at the 256 x 256 tile)
HEADS_ROUTES = [((), True, "igemm8_bf16_128x256_dense"), (("igemm8=2",), False, "igemm8_bf16_256x256_lin"),
                (("igemm8=2",), True, "igemm8_bf16_256x256_dense"), (("igemm8=4",), True, "igemm8_bf16_256x128_dense"),
                (("igemm2_tile=1",), True, "igemm2_bf16_256x64_dense"), (("igemm2_tile=2",), True, "igemm2_bf16_256x128_dense"),
                (("igemm2_tile=3",), True, "igemm2_bf16_256x256_dense"), (("no_igemm8",), True, "igemm2_bf16_256x128_dense")]


def head_major(y, tokens, dh=HEADS_DH):
    """[M][N] rows -> [B][N / dh][tokens][dh]."""
    M, N = y.shape
    return np.ascontiguousarray(y.reshape(M // tokens, tokens, N // dh, dh).transpose(0, 2, 1, 3))


def column_shift(N):
    """An integer per column that tells the 64-wide groups (and the columns within 16) apart: 16 (n / 64) + n % 16 - 48."""
    n = np.arange(N)
    return (16 * (n // 64) + n % 16 - 48).astype(F32)


@functools.lru_cache(maxsize=None)
def heads_case(mode, tokens, with_scale, seed=74):
    M, N, K = heads_batch(tokens) * tokens, HEADS_N, HEADS_K
    rng = rng_of(seed + (0 if mode == "int" else 1))
    if mode == "int":
        x, w = S.int_tensor(rng, (M, K), 2), S.pm1_rows(rng, N, K, 32)
        sc, sh = (S.int_scale(rng, N) if with_scale else None), column_shift(N)
    else:
        x, w = bf(rng.standard_normal((M, K))), bf(rng.standard_normal((N, K)) / np.sqrt(K))
        sc, sh = (S.gauss_scale(rng, N) if with_scale else None), (0.1 * rng.standard_normal(N)).astype(F32)
    ref, mag = S.gemm_ref(x, w, sc, sh, None, 0)
    if mode == "int":
        S.prove_exact(f"heads/{tokens}", ref, mag, [w], stored=[x, w])
        assert len({tuple(sh[g * 64:(g + 1) * 64]) for g in range(N // 64)}) == N // 64
    ref, mag = head_major(ref, tokens), head_major(mag, tokens)
    _ro(x, w, sc, sh, ref, mag)
    return dict(x=x, w=w, scale=sc, shift=sh, ref=ref, mag=mag, M=M, N=N, K=K, tokens=tokens, kred=K)


HEADS_DEFECTS = ("token_major_store", "image_index_per_tile", "qkv_group_swap", "truncate_store")


def emu_heads(d, defect=None):
    """x . w^T * scale + shift in float32, stored head-major into a sentinel-filled [B][3H][tokens][dh] buffer (returned flat with a
    guard of 4096 behind it, which an out-of-image row of image_index_per_tile may reach)."""
    M, N, tokens, dh = d["M"], d["N"], d["tokens"], HEADS_DH
    v = _gemm32(d["x"], d["w"], 64)
    v = (v if d["scale"] is None else v * np.asarray(d["scale"], F32)) + np.asarray(d["shift"], F32)
    y = bf16_truncate(v) if defect == "truncate_store" else bf(v)
    buf = np.full(M * N + 4096, SENTINEL, F32)
    if defect == "token_major_store":
        buf[:M * N] = y.reshape(-1)
        return buf
    m = np.arange(M)
    b = (m // 256 * 256) // tokens if defect == "image_index_per_tile" else m // tokens
    t = m - b * tokens
    g = np.arange(N) // dh
    if defect == "qkv_group_swap":
        H = N // dh // 3
        g = np.where((g >= H) & (g < 2 * H), g + H, np.where(g >= 2 * H, g - H, g))
    idx = ((b[:, None] * (N // dh) + g[None, :]) * tokens + t[:, None]) * dh + (np.arange(N) % dh)[None, :]
    ok = idx < buf.size
    buf[idx[ok]] = y[ok]
    return buf


# mv_linear_lnin_fwd with tokens > 0: tests/_strict_lngemm.py: LNFOLD_TOKEN_CASE (197 x 97 rows; no LNFOLD_CASES row is a multiple of 197)
# ================================================================================================ mv_vit_cls_pos_fwd
CLS_POS_CASES = [(768, "bf16"), (768, "fp32"), (200, "bf16"), (200, "fp32")]
CLS_B, CLS_T = 3, 5


@functools.lru_cache(maxsize=None)
def cls_pos_case(D, seed=75):
    rng = rng_of(seed + D)
    cls, pos = rng.standard_normal(D).astype(F32), rng.standard_normal((CLS_T, D)).astype(F32)
    ref = cls.astype(F64) + pos[0].astype(F64)
    mag = np.abs(cls).astype(F64) + np.abs(pos[0]).astype(F64)
    _ro(cls, pos, ref, mag)
    return cls, pos, ref, mag


def emu_cls_pos(cls, pos, out, defect=None):
    """tokens[b][0] = cls + pos[0] (one fp32 add, the store); every other row keeps the sentinel.  Defects: pos_off_by_one (pos[1]),
    stride_ignored (rows b instead of b tok_stride), truncate_store."""
    y = np.full((CLS_B * CLS_T, cls.shape[0]), SENTINEL, F32)
    v = np.asarray(cls, F32) + np.asarray(pos, F32)[1 if defect == "pos_off_by_one" else 0]
    v = np.asarray(v, F32) if out == "fp32" else (bf16_truncate(v) if defect == "truncate_store" else bf(v))
    y[np.arange(CLS_B) * (1 if defect == "stride_ignored" else CLS_T)] = v
    return y.reshape(CLS_B, CLS_T, -1)
