"""`-m gpu`: exact-integer and per-element parity checks of the MFMA conv / GEMM kernels (instruments: tests/_strict.py).

Every case names the kernel it must reach (`_lib.last_kernel()`, printed; a mismatch fails like `_cases.expect_kernel`) and prints
the worst |got - ref| / bound ratio, the rounding bias and the element counts (`pytest -s`).

Instrument 1 (mode "int", bit equality) runs on every kernel family below.  Instrument 2 (mode "gauss": the per-element bound
on every element, plus the rounding bias where K_red <= 1152, the output is bf16 and >= 4096 elements have |ref| >= 2^-6) runs
where the reference is rigorous: single-stage kernels, and two-stage kernels whose intermediate IS stored -- their second stage's
reference is computed from the kernel's own stored intermediate.  `bneck_tail`, `shuffle_dwpw`, `chain_rc` and `chain_rc0` never
store their intermediate: instrument 1 only.  Split-K: instrument 1 only (equality holds whatever the hand-over order).
No bias verdict (printed as `bias +nan over 0`; the per-element bound still applies): every fp32-output case (the 1x1 and
`*_res_f32out` conv shapes, stream 128_200, skinny 1x512x104, fc_stream 130x8192x260, fp32 compute mode), split-K (instrument 1
only), and the cases whose reference has fewer than 4096 elements of |ref| >= 2^-6: the 1 x 13 x 10 stride-2 conv shape (2240
outputs) and every skinny case (at most 1386 outputs).

Kernels that take host-folded operands get them from the packers the models use (ops._res_fragments, ops._rc_shift_rows,
ops.dwpw_fragments); BatchNorm scales folded into bf16 rows and the two-term bf16 shift rows (header: "hi + lo = v to 16 mantissa
bits") are operands here: the reference reads the same folded values, so no term is added to the bound for them.

Shapes are the smallest that reach the kernel with a ragged M tail, a ragged N tail and >= 2 reduction steps; where a dispatch gate
needs more rows the case says which.  Out of scope (outputs not exactly representable; a separate derivation is needed): the
LayerNorm- and GELU-bearing kernels (`ln_*`, `cnblock`, `mv_swin_block_attn_fwd`).  Every activation beyond none / ReLU that
these kernels fuse runs in tests/test_strict_act_gpu.py, on the runners this module shares with it (tests/_strict_gpu.py).  The
softmax attention kernels (`mha_*`, `swin_attn_*`) are covered in tests/test_strict_attn_gpu.py.
"""
import numpy as np
import pytest
import torch

from eqxvision_amd import _lib, ops
from tests import _strict as S
from tests._strict_gpu import (DT, _dev, _Flags, _host, _need_gpu, _out, _p, _stream,  # noqa: F401  (_need_gpu: the module fixture)
                               _run_conv, _run_dwconv, _run_fc_stream, _run_stem_nchw, _sc, _sh, _verdict, _w, _x)

pytestmark = pytest.mark.gpu

BF, F32 = _lib.BF16, _lib.F32


def _shift_operand(h):
    """The value the two-term bf16 shift rows carry (ops._rc_shift_rows; header: hi + lo = v to 16 mantissa bits)."""
    t = torch.from_numpy(np.asarray(h, np.float32))
    hi = t.to(torch.bfloat16)
    lo = (t - hi.float()).to(torch.bfloat16)
    return hi.double().numpy() + lo.double().numpy()


# ================================================================================================ mv_conv2d_nhwc_fwd / mv_linear_fwd
# (N, H, W, C, K, R, stride, pad, dil), act, res, out
CONV_SHAPES = {
    "3x3_64_72": ((2, 9, 11, 64, 72, 3, 1, 1, 1), 1, False, "bf16"),
    "3x3_s2_128_64_res": ((1, 13, 10, 128, 64, 3, 2, 1, 1), 0, True, "bf16"),
    "1x1_192_264_res_f32out": ((3, 7, 7, 192, 264, 1, 1, 0, 1), 1, True, "fp32"),
    "3x3_dil2_64_128": ((1, 13, 11, 64, 128, 3, 1, 2, 2), 0, False, "bf16"),
    "3x3_64_72_res_f32out": ((2, 9, 11, 64, 72, 3, 1, 1, 1), 1, True, "fp32"),      # the fp32-output instances of the conv kernels
}
# flag -> kernel per shape (order of CONV_SHAPES); the 128-row tiles serve these small shapes by default
# (`no_igemm2`, `no_stream` and `igemm2_tile` change nothing below M = 4096: they run where they change the dispatch, further down)
_T128 = ["igemm_bf16_128x128_conv", "igemm_bf16_128x64_conv", "igemm_bf16_128x128_dense", "igemm_bf16_128x128_conv",
         "igemm_bf16_128x128_conv"]
_T64 = ["igemm_bf16_128x64_conv", "igemm_bf16_128x64_conv", "igemm_bf16_128x64_dense", "igemm_bf16_128x64_conv", "igemm_bf16_128x64_conv"]


def _g8(tile):
    return [f"igemm8_bf16_{tile}_conv", f"igemm8_bf16_{tile}_conv", f"igemm8_bf16_{tile}_dense_f32out", f"igemm8_bf16_{tile}_conv",
            f"igemm8_bf16_{tile}_conv_f32out"]


CONV_FLAGS = {
    "default": _T128,
    "igemm_tile=1": ["igemm_bf16_128x128_conv", "igemm_bf16_128x128_conv", "igemm_bf16_128x128_dense", "igemm_bf16_128x128_conv",
                     "igemm_bf16_128x128_conv"],
    "igemm_tile=2": _T64,
    "igemm8=2": _g8("256x256"), "igemm8=3": _g8("128x256"), "igemm8=4": _g8("256x128"),
    "force_generic": ["conv_generic"] * 5,
}
CONV_CASES = [(f"{s}/{f}", s, f, CONV_FLAGS[f][i]) for i, s in enumerate(CONV_SHAPES) for f in CONV_FLAGS]


@pytest.mark.parametrize("mode", ["int", "gauss"])
@pytest.mark.parametrize("tag,shape,flag,expect", CONV_CASES, ids=[c[0] for c in CONV_CASES])
def test_conv_nhwc(tag, shape, flag, expect, mode):
    sh, act, res, out = CONV_SHAPES[shape]
    _run_conv(f"conv/{tag}/{mode}", mode, sh, expect, act=act, res=res, out=out, flags=() if flag == "default" else (flag,), seed=11)


# igemm2 (256-row tiles): igemm2_wanted gates it on M >= 4096 AND R * S * (C / 64) >= 4 k-tiles, forced tiles included.  So the
# four channel shapes run at 4096 + 34 output pixels (1 x 59 x 70; the stride-2 one at 4 x 33 x 33 = 4096 + 260), and the 1x1 shape
# takes C = 256 instead of 192 (192 / 64 = 3 k-tiles do not pass the gate).  The same maps also carry the flags that only change
# the dispatch up here: the default rule (256x128), `no_igemm2` (back on the 128-row tile) and, on the c3x3c64 shape of the next
# test (M >= 8192), `no_stream` (igemm2 instead of conv3x3c64_halo).
_BIG = {"3x3_64_72": ((1, 59, 70, 64, 72, 3, 1, 1, 1), 1, False, "bf16"),
        "3x3_s2_128_64_res": ((4, 65, 66, 128, 64, 3, 2, 1, 1), 0, True, "bf16"),
        "1x1_256_264_res_f32out": ((1, 59, 70, 256, 264, 1, 1, 0, 1), 1, True, "fp32"),
        "3x3_dil2_64_128": ((1, 59, 70, 64, 128, 3, 1, 2, 2), 0, False, "bf16"),
        "3x3_64_72_res_f32out": ((1, 59, 70, 64, 72, 3, 1, 1, 1), 1, True, "fp32"),
        "3x3_64_64_c3_shape": ((69, 12, 10, 64, 64, 3, 1, 1, 1), 1, False, "bf16")}
IGEMM2_CASES = [(f"{s}/igemm2_tile={t}", *_BIG[s], f"igemm2_tile={t}", f"igemm2_bf16_{tile}_{'dense' if s.startswith('1x1') else 'conv'}")
                for s in ("3x3_64_72", "3x3_s2_128_64_res", "1x1_256_264_res_f32out", "3x3_dil2_64_128", "3x3_64_72_res_f32out")
                for t, tile in ((1, "256x64"), (3, "256x256"))] + [
    ("3x3_64_72/default", *_BIG["3x3_64_72"], None, "igemm2_bf16_256x128_conv"),
    ("3x3_64_72/no_igemm2", *_BIG["3x3_64_72"], "no_igemm2", "igemm_bf16_128x128_conv"),
    ("3x3_64_64_c3_shape/no_stream", *_BIG["3x3_64_64_c3_shape"], "no_stream", "igemm2_bf16_256x64_conv"),
]


@pytest.mark.parametrize("mode", ["int", "gauss"])
@pytest.mark.parametrize("tag,sh,act,res,out,flag,expect", IGEMM2_CASES, ids=[c[0] for c in IGEMM2_CASES])
def test_conv_igemm2(tag, sh, act, res, out, flag, expect, mode):
    _run_conv(f"igemm2/{tag}/{mode}", mode, sh, expect, act=act, res=res, out=out, flags=(flag,) if flag else (), seed=12)


# conv3x3c64_halo is gated on M >= 8192: 69 images of 12 x 10 (8280 rows), and a map wider than one 64-column tile
C3_CASES = [("69x12x10", (69, 12, 10, 64, 64, 3, 1, 1, 1)), ("2x37x112_wide", (2, 37, 112, 64, 64, 3, 1, 1, 1))]


@pytest.mark.parametrize("mode", ["int", "gauss"])
@pytest.mark.parametrize("tag,sh", C3_CASES, ids=[c[0] for c in C3_CASES])
def test_c3x3c64(tag, sh, mode):
    _run_conv(f"c3x3c64/{tag}/{mode}", mode, sh, "conv3x3c64_halo", act=1, seed=13)


# stream1x1 / stream_narrow are gated on M >= 8192: M = 8192 + 37 rows through mv_linear_fwd.  (C, K, res, out, nnz, kernel)
STREAM_CASES = [(64, 256, True, "bf16", 32, "stream1x1_bf16_bn128_k64"), (16, 96, False, "bf16", 8, "stream1x1_bf16_bn128_k16"),
                (24, 144, False, "bf16", 8, "stream1x1_bf16_bn128_k24"), (144, 24, True, "bf16", 32, "stream1x1_bf16_bn64_k144"),
                (128, 200, True, "fp32", 32, "stream1x1_bf16_bn128_k128"),
                (64, 256, True, "bf16", 32, "igemm_bf16_128x128_dense")]           # the last row under `no_stream`: the tile kernel instead


@pytest.mark.parametrize("mode", ["int", "gauss"])
@pytest.mark.parametrize("C,K,res,out,nnz,expect", STREAM_CASES, ids=[f"{c[0]}_{c[1]}" + ("_no_stream" if c[5].startswith("igemm_") else "") for c in STREAM_CASES])
def test_stream1x1(C, K, res, out, nnz, expect, mode):
    flags = ("no_stream",) if expect.startswith("igemm_") else ()
    _run_conv(f"stream/{C}_{K}{'/no_stream' if flags else ''}/{mode}", mode, (1, 8192 + 37, 1, C, K, 1, 1, 0, 1), expect, act=1, res=res,
              out=out, linear=True, nnz=nnz, flags=flags, seed=14)


# the skinny kernel sits behind the implicit-GEMM gate (reduction a multiple of 64, outputs a multiple of 8): 33 x 64 x 40 and
# 17 x 192 x 64 reach it; the issue's 33 x 64 x 42 and 17 x 144 x 64 are kept, pinned to the kernels the dispatch gives them
SKINNY_CASES = [(33, 64, 40, "bf16", 1, "skinny_linear_mfma"), (17, 192, 64, "bf16", 0, "skinny_linear_mfma"),
                (1, 512, 104, "fp32", 0, "skinny_linear_mfma"), (33, 64, 42, "bf16", 1, "conv_generic"),
                (17, 144, 64, "bf16", 0, "igemm_bf16_128x64_dense_oddc")]


@pytest.mark.parametrize("mode", ["int", "gauss"])
@pytest.mark.parametrize("M,Kr,N,out,act,expect", SKINNY_CASES, ids=[f"{c[0]}x{c[1]}x{c[2]}" for c in SKINNY_CASES])
def test_skinny(M, Kr, N, out, act, expect, mode):
    _run_conv(f"skinny/{M}x{Kr}x{N}/{mode}", mode, (1, M, 1, Kr, N, 1, 1, 0, 1), expect, act=act, out=out, linear=True, seed=15)


def test_splitk_linear_exact():
    _run_conv("splitk/linear_3136x832x512", "int", (1, 3136, 1, 832, 512, 1, 1, 0, 1), "igemm8_bf16_128x256_dense_splitk", act=1, res=True,
              linear=True, splitk=True, flags=("splitk_min_nk=12",), seed=16)


def test_splitk_conv_exact():
    _run_conv("splitk/conv_64x7x7_512_512_3x3", "int", (64, 7, 7, 512, 512, 3, 1, 1, 1), "igemm8_bf16_128x256_conv_splitk", act=1, res=True,
              splitk=True, xlim=1, seed=17)


# fp32 compute mode: the shapes of the f32/* cases of _cases.py, shrunk (conv_f32_lds_mfma is gated on M >= 1024: 6 x 14 x 14 = 1176)
F32_CASES = [("conv3x3_c24_k40_direct", (1, 15, 13, 24, 40, 3, 1, 1, 1), 1, False, False, 16, "conv_f32_mfma"),
             ("conv3x3_s2_c128_k96_res_lds", (6, 28, 28, 128, 96, 3, 2, 1, 1), 1, True, False, 32, "conv_f32_lds_mfma"),
             ("linear_33x96x288_skinny", (1, 33, 1, 96, 288, 1, 1, 0, 1), 0, False, True, 32, "skinny_linear_f32_mfma")]


@pytest.mark.parametrize("mode", ["int", "gauss"])
@pytest.mark.parametrize("tag,sh,act,res,linear,nnz,expect", F32_CASES, ids=[c[0] for c in F32_CASES])
def test_f32_compute(tag, sh, act, res, linear, nnz, expect, mode):
    _run_conv(f"f32/{tag}/{mode}", mode, sh, expect, act=act, res=res, dtype="fp32", out="fp32", linear=linear, nnz=nnz, seed=18)


# ================================================================================================ mv_fc_stream_fwd
# (M, K, N, bias).  The second row is the issue's 130 x 640 x 260: the gate N * K >= 2^21 forces K = 8192 at N = 260.
FC_CASES = [(3, 1024, 4096, True, "bf16"), (130, 8192, 260, False, "fp32")]


@pytest.mark.parametrize("mode", ["int", "gauss"])
@pytest.mark.parametrize("M,K,N,bias,out", FC_CASES, ids=[f"{c[0]}x{c[1]}x{c[2]}" for c in FC_CASES])
def test_fc_stream(M, K, N, bias, out, mode):
    _run_fc_stream(M, K, N, bias, out, mode)


# ================================================================================================ fused ResNet kernels
def _stage1(mode, rng, M, cins, K, fold, res, xlim=1, nnz=4, hlim=2, rlim=4, relu_in=False):
    """x sources (M, C_i), one weight matrix per source with its BatchNorm scale, one summed shift, optional residual.
    `fold`: the scales are folded into bf16 weight rows on the host (the reference then reads the folded rows)."""
    xs = [np.maximum(_x(mode, rng, (M, c), xlim), 0 if relu_in else -np.inf).astype(np.float32) for c in cins]
    ws = [_w(mode, rng, K, c, nnz) for c in cins]
    ss = [_sc(mode, rng, K) for _ in cins]
    h = _sh(mode, rng, K, hlim)
    r = None
    if res:
        r = S.int_tensor(rng, (M, K), rlim) if mode == "int" else S.bf(rng.standard_normal((M, K)))
    if fold:
        wcat = S.bf(np.concatenate([w * s[:, None] for w, s in zip(ws, ss)], axis=1))
        return xs, wcat, None, h, r
    assert len(cins) == 1
    return xs, ws[0], ss[0], h, r


def _two_stage_verdict(tag, kern, expect, mode, xs, w, sc, h, r, w1, s1, h1, y_got, t1_got, y_rows=None, hidden_y=None):
    """Stage 1 against float64 of the operands; stage 2 against float64 of the kernel's OWN stored y (mode gauss) -- in mode int
    the reference chain is exact, so y and t1 are both compared with it.  `y_rows`: the rows of the full map that y holds."""
    xcat = np.concatenate(xs, axis=1)
    yref, ymag = S.gemm_ref(xcat, w, sc, h, r, 1)
    parts = []
    if mode == "int":
        t1ref, t1mag = S.gemm_ref(yref, w1, s1, h1, None, 1)
        S.prove_exact(tag, yref, ymag, [w], stored=list(xs) + [w, w1] + ([r] if r is not None else []))
        S.prove_exact(tag + " t1", t1ref, t1mag, [w1], hidden=[yref])
        if y_got is not None:
            parts.append(("y", y_got, yref if y_rows is None else yref[y_rows], None, 0, "bf16"))
        parts.append(("t1", t1_got, t1ref, None, 0, "bf16"))
    else:
        if y_got is not None:
            sel = slice(None) if y_rows is None else y_rows
            parts.append(("y", y_got, yref[sel], ymag[sel], xcat.shape[1], "bf16"))
            t1ref, t1mag = S.gemm_ref(y_got, w1, s1, h1, None, 1)           # from the kernel's own stored intermediate
            parts.append(("t1", t1_got[sel], t1ref, t1mag, w1.shape[1], "bf16"))
    _verdict(tag, kern, expect, mode, parts)


CHAIN_CASES = [(64, 256, 64, 8192, "chain1x1_bf16_64_256_64"), (64, 256, 64, 8192 + 37, "chain1x1_bf16_64_256_64"),
               (64, 256, 128, 8192 + 37, "chain1x1_bf16_64_256_128"),
               (128, 512, 128, 16384 + 37, "chain_stream_bf16_128_512_128")]        # gates: M >= 8192; the streamed one M >= 16384


@pytest.mark.parametrize("mode", ["int", "gauss"])
@pytest.mark.parametrize("C,K,N2,M,expect", CHAIN_CASES, ids=[f"{c[0]}_{c[1]}_{c[2]}_M{c[3]}" for c in CHAIN_CASES])
def test_chain(C, K, N2, M, expect, mode):
    rng = S.rng_of(31)
    assert _lib.load().mv_conv1x1_chain_supported(M, C, K, N2, BF)
    xs, w3, s3, h3, r = _stage1(mode, rng, M, [C], K, False, True, nnz=8)
    w1, s1, h1 = _w(mode, rng, N2, K, 4), _sc(mode, rng, N2), _sh(mode, rng, N2)
    d = [_dev(a) for a in (xs[0], w3, r, w1)]
    f = [_dev(a, "fp32") for a in (s3, h3, s1, h1)]
    y, t1 = _out((M, K)), _out((M, N2))
    _lib.call("mv_conv1x1_chain_fwd", _p(d[0]), _p(d[1]), _p(f[0]), _p(f[1]), _p(d[2]), _p(y), _p(d[3]), _p(f[2]), _p(f[3]), _p(t1), M, C, K, N2,
              BF, _stream())
    kern = _lib.last_kernel()
    torch.cuda.synchronize()
    _two_stage_verdict(f"chain/{C}_{K}_{N2}_M{M}/{mode}", kern, expect, mode, xs, w3, s3, h3, r, w1, s1, h1, _host(y), _host(t1))


def _even_rows(N, H, W):
    idx = np.arange(N * H * W).reshape(N, H, W)
    return idx[:, ::2, ::2].reshape(-1)


@pytest.mark.parametrize("mode", ["int", "gauss"])
def test_chain_sub(mode):
    """y written at even (h, w) only: those rows of y are checked, and (mode gauss) t1 at the rows whose y the kernel stored.
    10 images of 28 x 30 = 8400 rows: the gate is M >= 8192."""
    N, H, W, C, K, N2 = 10, 28, 30, 64, 256, 128
    M = N * H * W
    rng = S.rng_of(32)
    assert _lib.load().mv_conv1x1_chain_sub_supported(N, H, W, C, K, N2, BF)
    xs, w3, s3, h3, r = _stage1(mode, rng, M, [C], K, False, True, nnz=8)
    w1, s1, h1 = _w(mode, rng, N2, K, 4), _sc(mode, rng, N2), _sh(mode, rng, N2)
    d = [_dev(a) for a in (xs[0], w3, r, w1)]
    f = [_dev(a, "fp32") for a in (s3, h3, s1, h1)]
    nsub = N * (H // 2) * (W // 2)
    ybuf, t1 = _out((nsub * K + 4096,)), _out((M, N2))
    _lib.call("mv_conv1x1_chain_sub_fwd", _p(d[0]), _p(d[1]), _p(f[0]), _p(f[1]), _p(d[2]), _p(ybuf), _p(d[3]), _p(f[2]), _p(f[3]), _p(t1),
              N, H, W, C, K, N2, BF, _stream())
    kern = _lib.last_kernel()
    torch.cuda.synchronize()
    assert bool((ybuf[nsub * K:] == -7.0).all()), "guard band behind the compact y touched"
    rows = _even_rows(N, H, W)
    t1h = _host(t1)
    _two_stage_verdict(f"chain_sub/{mode}", kern, "chain1x1_bf16_64_256_128_ysub2", mode, xs, w3, s3, h3, r, w1, s1, h1,
                           _host(ybuf[:nsub * K]).reshape(nsub, K), t1h, y_rows=rows)


@pytest.mark.parametrize("mode", ["int", "gauss"])
@pytest.mark.parametrize("M", [8192, 8192 + 37])
def test_dual_chain(M, mode):
    C, K, N2 = 64, 256, 64
    rng = S.rng_of(33)
    assert _lib.load().mv_conv1x1_dual_chain_supported(M, C, C, K, N2, BF)
    xs, wcat, _, h, _ = _stage1(mode, rng, M, [C, C], K, True, False)
    w1, s1, h1 = _w(mode, rng, N2, K, 4), _sc(mode, rng, N2), _sh(mode, rng, N2)
    d = [_dev(a) for a in (xs[0], xs[1], wcat, w1)]
    f = [_dev(a, "fp32") for a in (h, s1, h1)]
    y, t1 = _out((M, K)), _out((M, N2))
    _lib.call("mv_conv1x1_dual_chain_fwd", _p(d[0]), _p(d[1]), _p(d[2]), None, _p(f[0]), _p(y), _p(d[3]), _p(f[1]), _p(f[2]), _p(t1), M, C, C, K,
              N2, BF, _stream())
    kern = _lib.last_kernel()
    torch.cuda.synchronize()
    _two_stage_verdict(f"dual_chain/M{M}/{mode}", kern, "chain1x1_dual_bf16_64+64_256_64", mode, xs, wcat, None, h, None, w1, s1, h1,
                       _host(y), _host(t1))


# mv_conv1x1_dual_fwd is gated on M >= 4096: 5 images of 28 x 30 = 4200 output pixels, the second source strided
@pytest.mark.parametrize("mode", ["int", "gauss"])
@pytest.mark.parametrize("stride,C1,C2,K,flag,expect", [(2, 64, 128, 200, None, "igemm2_dual_bf16_256x128"),
                                                       (1, 64, 64, 72, None, "igemm2_dual_bf16_256x128"),
                                                       (2, 64, 128, 200, "igemm8=2", "igemm8_dual_bf16_256x256")],
                         ids=["s2_64+128_200", "s1_64+64_72", "s2_64+128_200_igemm8"])
def test_dual(stride, C1, C2, K, flag, expect, mode):
    N, Ho, Wo = 5, 28, 30
    M = N * Ho * Wo
    H2, W2 = (Ho - 1) * stride + 1 + (stride - 1), (Wo - 1) * stride + 1
    rng = S.rng_of(34)
    assert _lib.load().mv_conv1x1_dual_supported(M, C1, C2, K, BF)
    x = _x(mode, rng, (N, Ho, Wo, C1), 2)
    x2 = _x(mode, rng, (N, H2, W2, C2), 2)
    w3, wd = _w(mode, rng, K, C1, 16), _w(mode, rng, K, C2, 16)
    wcat = S.bf(np.concatenate([w3 * _sc(mode, rng, K)[:, None], wd * _sc(mode, rng, K)[:, None]], axis=1))
    h = _sh(mode, rng, K)
    xcat = np.concatenate([x.reshape(M, C1), x2[:, ::stride, ::stride][:, :Ho, :Wo].reshape(M, C2)], axis=1)
    ref, mag = S.gemm_ref(xcat, wcat, None, h, None, 1)
    if mode == "int":
        S.prove_exact("dual", ref, mag, [wcat], stored=[x, x2, wcat])
    xd, x2d, wd_, hd = _dev(x), _dev(x2), _dev(wcat), _dev(h, "fp32")
    y = _out((M, K))
    with _Flags((flag,) if flag else ()):
        _lib.call("mv_conv1x1_dual_fwd", _p(xd), _p(x2d), _p(wd_), None, _p(hd), _p(y), N, Ho, Wo, C1, H2, W2, C2, stride, K, 1, BF, _stream())
        kern = _lib.last_kernel()
    torch.cuda.synchronize()
    _verdict(f"dual/s{stride}_{C1}+{C2}_{K}/{mode}", kern, expect, mode, [("y", _host(y), ref, mag, C1 + C2, "bf16")])


def _acc_operands(mode, rng, M, cins, K, N2, res):
    """Operands of the accumulator-layout kernels: scales folded into bf16 rows, fragments by ops._res_fragments, shifts as the
    two-term bf16 rows of ops._rc_shift_rows (the reference reads hi + lo, the value the rows carry)."""
    xs, wy, _, h, r = _stage1(mode, rng, M, cins, K, True, res, relu_in=True)
    w1 = S.bf(_w(mode, rng, N2, K, 4) * _sc(mode, rng, N2)[:, None])
    h1 = _sh(mode, rng, N2)
    wf = torch.from_numpy(ops._res_fragments(wy, w1).reshape(-1)).to(torch.bfloat16).cuda()
    sh = torch.from_numpy(ops._rc_shift_rows(h, h1).view(np.int32)).cuda()
    return xs, wy, _shift_operand(h), r, w1, _shift_operand(h1), wf, sh


# chain_res (C = 64): gate M >= 8192 -> 10 images of 28 x 30; chain_l2 (C = 128, weights streamed): gate M >= 16384 -> 20 images
CHAIN_RES_CASES = [(10, 64, 256, 128, 0, "chain_res_bf16_64_256_128"), (10, 64, 256, 128, 2, "chain_res_bf16_64_256_128_ysub2"),
                   (20, 128, 512, 128, 2, "chain_l2_res_bf16_128_512_128_ysub2"), (20, 128, 512, 256, 0, "chain_l2_exit_bf16_128_512_256")]


@pytest.mark.parametrize("mode", ["int", "gauss"])
@pytest.mark.parametrize("N,C,K,N2,sub,expect", CHAIN_RES_CASES, ids=[c[5] for c in CHAIN_RES_CASES])
def test_chain_res(N, C, K, N2, sub, expect, mode):
    H, W = 28, 30
    M = N * H * W
    rng = S.rng_of(35)
    assert _lib.load().mv_conv1x1_chain_res_supported(N, H, W, C, K, N2, sub, BF)
    xs, wy, h, r, w1, h1, wf, sh = _acc_operands(mode, rng, M, [C], K, N2, True)
    t2d, rd = _dev(xs[0]), _dev(r)
    ny = (N * (H // 2) * (W // 2) if sub else M)
    ybuf, t1 = _out((ny * K + 4096,)), _out((M, N2))
    _lib.call("mv_conv1x1_chain_res_fwd", _p(t2d), _p(rd), _p(wf), _p(sh), _p(ybuf), _p(t1), N, H, W, C, K, N2, sub, BF, _stream())
    kern = _lib.last_kernel()
    torch.cuda.synchronize()
    assert bool((ybuf[ny * K:] == -7.0).all()), "guard band behind y touched"
    _two_stage_verdict(f"chain_res/{expect}/{mode}", kern, expect, mode, xs, wy, None, h, r, w1, None, h1,
                       _host(ybuf[:ny * K]).reshape(ny, K), _host(t1), y_rows=_even_rows(N, H, W) if sub else None)


@pytest.mark.parametrize("mode", ["int", "gauss"])
def test_dual_chain_res(mode):
    """chain_l2 entry (mv_conv1x1_dual_chain_res_fwd): gate M >= 16384; 16384 + 37 rows."""
    M, C1, C2, K, N2 = 16384 + 37, 128, 256, 512, 128
    rng = S.rng_of(36)
    assert _lib.load().mv_conv1x1_dual_chain_res_supported(M, C1, C2, K, N2, BF)
    xs, wy, h, _, w1, h1, wf, sh = _acc_operands(mode, rng, M, [C1, C2], K, N2, False)
    d = [_dev(a) for a in xs]
    y, t1 = _out((M, K)), _out((M, N2))
    _lib.call("mv_conv1x1_dual_chain_res_fwd", _p(d[0]), _p(d[1]), _p(wf), _p(sh), _p(y), _p(t1), M, C1, C2, K, N2, BF, _stream())
    kern = _lib.last_kernel()
    torch.cuda.synchronize()
    _two_stage_verdict(f"dual_chain_res/{mode}", kern, "chain_l2_entry_bf16_128+256_512_128", mode, xs, wy, None, h, None, w1, None, h1,
                       _host(y), _host(t1))


@pytest.mark.parametrize("M", [8192, 8192 + 37])
def test_chain_rc_exact(M):
    """mv_conv1x1_chain_rc_fwd and mv_conv1x1_chain_rc0_fwd: y0 is recomputed and never stored -> instrument 1 only.  Gate M >= 8192."""
    C, K, N2 = 64, 256, 64
    rng = S.rng_of(37)
    assert _lib.load().mv_conv1x1_chain_rc_supported(M, C, K, N2, BF)
    t20, x0, t21 = (np.maximum(S.int_tensor(rng, (M, C), 1), 0) for _ in range(3))
    wcat = np.concatenate([S.pm1_rows(rng, K, C, 4) * S.int_scale(rng, K, (1,))[:, None] for _ in range(2)], axis=1)
    w31 = S.pm1_rows(rng, K, C, 4) * S.int_scale(rng, K)[:, None]
    h0, h31 = S.int_tensor(rng, (K,), 2), S.int_tensor(rng, (K,), 2)
    w1a, w1n = (S.pm1_rows(rng, N2, K, 4) * S.int_scale(rng, N2)[:, None] for _ in range(2))
    h1a, h1n = S.int_tensor(rng, (N2,), 8), S.int_tensor(rng, (N2,), 8)
    y0, m0 = S.gemm_ref(np.concatenate([t20, x0], 1), wcat, None, h0, None, 1)
    y1, m1 = S.gemm_ref(t21, w31, None, h31, y0, 1)
    t1, mt = S.gemm_ref(y1, w1n, None, h1n, None, 1)
    ta, ma = S.gemm_ref(y0, w1a, None, h1a, None, 1)
    S.prove_exact("rc y0", y0, m0, [wcat], stored=[t20, x0, t21, wcat, w31, w1a, w1n])
    S.prove_exact("rc y1", y1, m1, [w31], hidden=[y0])
    S.prove_exact("rc t1", t1, mt, [w1n], hidden=[y1])
    S.prove_exact("rc0 t1", ta, ma, [w1a], hidden=[y0])
    wf = torch.from_numpy(ops._res_fragments(np.concatenate([wcat, w31], 1), w1n).reshape(-1)).to(torch.bfloat16).cuda()
    sh = torch.from_numpy(ops._rc_shift_rows(h0, h31, h1n).view(np.int32)).cuda()
    wf0 = torch.from_numpy(ops._res_fragments(wcat, w1a).reshape(-1)).to(torch.bfloat16).cuda()
    sh0 = torch.from_numpy(ops._rc_shift_rows(h0, h1a).view(np.int32)).cuda()
    d = [_dev(a) for a in (t21, t20, x0)]
    yd, td, tc = _out((M, K)), _out((M, N2)), _out((M, N2))
    _lib.call("mv_conv1x1_chain_rc_fwd", _p(d[0]), _p(d[1]), _p(d[2]), _p(wf), _p(sh), _p(yd), _p(td), M, C, K, N2, BF, _stream())
    kern = _lib.last_kernel()
    _lib.call("mv_conv1x1_chain_rc0_fwd", _p(d[1]), _p(d[2]), _p(wf0), _p(sh0), _p(tc), M, C, K, N2, BF, _stream())
    kern0 = _lib.last_kernel()
    torch.cuda.synchronize()
    _verdict(f"chain_rc/M{M}", kern, "chain_rc1_bf16_64x3_256_64", "int", [("y1", _host(yd), y1, None, 0, "bf16"), ("t1", _host(td), t1, None, 0, "bf16")])
    _verdict(f"chain_rc0/M{M}", kern0, "chain_rc0_bf16_64x2_256_64", "int", [("t1", _host(tc), ta, None, 0, "bf16")])


@pytest.mark.parametrize("B", [1, 3])
def test_bneck_tail_exact(B):
    """mv_bottleneck_tail_fwd: the 256-channel intermediate stays in LDS -> instrument 1 only (14 x 14 x 256 -> 1024 is the only shape)."""
    HW, WID, COUT = 14, 256, 1024
    rng = S.rng_of(38 + B)
    assert _lib.load().mv_bottleneck_tail_supported(HW, HW, WID, COUT, BF)
    t1 = np.maximum(S.int_tensor(rng, (B, HW, HW, WID), 1), 0)
    w2 = S.pm1_rows(rng, WID, 9 * WID, 9).reshape(WID, 3, 3, WID)                  # KRSC
    s2, h2 = S.int_scale(rng, WID), S.int_tensor(rng, (WID,), 2)
    w3 = S.pm1_rows(rng, COUT, WID, 4)
    s3, h3 = S.int_scale(rng, COUT), S.int_tensor(rng, (COUT,), 8)
    r = S.int_tensor(rng, (B, HW, HW, COUT), 16)
    t2, m2 = S.conv_ref(t1, w2, s2, h2, None, 1, 1, 1, 1)
    yref, my = S.gemm_ref(t2.reshape(-1, WID), w3, s3, h3, r.reshape(-1, COUT), 1)
    S.prove_exact("bneck t2", t2, m2, [w2], stored=[t1, w2, w3, r])
    S.prove_exact("bneck y", yref, my, [w3], hidden=[t2])
    w2f = w2.reshape(WID // 32, 32, 9, WID // 16, 2, 8).transpose(0, 2, 3, 4, 1, 5)             # the fragment order of the header,
    w3f = w3.reshape(COUT // 256, 8, 32, WID // 16, 2, 8).transpose(0, 1, 3, 4, 2, 5)           # as ops.prep_bneck_tail lays it out
    d = [_dev(a) for a in (t1, w2f, w3f, r)]
    f = [_dev(a, "fp32") for a in (s2, h2, s3, h3)]
    y = _out((B, HW, HW, COUT))
    _lib.call("mv_bottleneck_tail_fwd", _p(d[0]), _p(d[1]), _p(f[0]), _p(f[1]), _p(d[2]), _p(f[2]), _p(f[3]), _p(d[3]), _p(y), B, HW, HW, WID, COUT,
              BF, _stream())
    kern = _lib.last_kernel()
    torch.cuda.synchronize()
    _verdict(f"bneck_tail/B{B}", kern, "bneck_tail_bf16_14x14_256_1024", "int", [("y", _host(y).reshape(-1, COUT), yref, None, 0, "bf16")])


# ================================================================================================ grouped / depthwise
@pytest.mark.parametrize("mode", ["int", "gauss"])
@pytest.mark.parametrize("N,H,W,C,groups,res", [(2, 9, 11, 128, 32, False), (2, 9, 9, 104, 13, True)], ids=["128_g32", "104_g13_9x9_res"])
def test_grouped64(N, H, W, C, groups, res, mode):
    cg = C // groups
    rng = S.rng_of(41)
    lib = _lib.load()
    assert lib.mv_conv2d_grouped64_supported(C, C, 3, 3, groups, BF, BF)
    x = _x(mode, rng, (N, H, W, C), 2)
    w = np.concatenate([_w(mode, rng, cg, 9 * cg, 12) for _ in range(groups)], 0).reshape(C, 3, 3, cg)           # K R S Cg
    sc, sh = _sc(mode, rng, C), _sh(mode, rng, C)
    r = None
    if res:
        r = S.int_tensor(rng, (N, H, W, C), 16) if mode == "int" else S.bf(rng.standard_normal((N, H, W, C)))
    ref, mag = S.conv_ref(x, w, sc, sh, r, 1, 1, 1, 1, groups)
    if mode == "int":
        S.prove_exact("grouped64", ref, mag, [w[g * cg:(g + 1) * cg] for g in range(groups)], stored=[x, w])
    win = int(lib.mv_conv2d_grouped64_window(C, groups))
    w64 = np.zeros((C, 3, 3, win), np.float32)
    for k in range(C):
        g0 = (k // cg) * cg - ((k // 64 * 64) // cg) * cg
        w64[k, :, :, g0:g0 + cg] = w[k]
    xd, wd, scd, shd, rd = _dev(x), _dev(w64), _dev(sc, "fp32"), _dev(sh, "fp32"), (None if r is None else _dev(r))
    y = _out((N, H, W, C))
    _lib.call("mv_conv2d_nhwc_grouped64_fwd", _p(xd), _p(wd), _p(scd), _p(shd), _p(rd), _p(y), N, H, W, C, C, 3, 3, 1, 1, 1, 1, 1, 1, groups, 1,
              BF, BF, _stream())
    kern = _lib.last_kernel()
    torch.cuda.synchronize()
    _verdict(f"grouped64/{C}_g{groups}/{mode}", kern, "igemm_grouped64_bf16_128x64", mode, [("y", _host(y), ref, mag, 9 * cg, "bf16")])


DW_CASES = [("3x3_s1_13x17_c40", 2, 13, 17, 40, 3, 1, None, "dwconv3x3_s1_bf16x8x4"), ("3x3_s2_15x21_c16", 3, 15, 21, 16, 3, 2, None, "dwconv3x3_s2_bf16x8x4"),
            ("5x5_9x21_c200", 3, 9, 21, 200, 5, 1, None, "dwconv5x5_s1_lds_tile"), ("3x3_tile3_flag", 2, 13, 17, 40, 3, 1, "dwconv_tile3", "dwconv3x3_s1_lds_tile"),
            ("5x5_no_tile_flag", 3, 9, 21, 200, 5, 1, "dwconv_no_tile", "dwconv5x5_s1_bf16x8x4")]


@pytest.mark.parametrize("mode", ["int", "gauss"])
@pytest.mark.parametrize("tag,N,H,W,C,R,stride,flag,expect", DW_CASES, ids=[c[0] for c in DW_CASES])
def test_dwconv(tag, N, H, W, C, R, stride, flag, expect, mode):
    _run_dwconv(tag, N, H, W, C, R, stride, flag, expect, mode)


# ================================================================================================ ShuffleNet: mv_shuffle_dwpw_fwd
DWPW_CASES = [(Cx, N, Nr, H, W, s, p) for (Cx, N, Nr) in ((120, 120, 116), (24, 24, 24)) for (H, W) in ((5, 5), (9, 13)) for s in (1, 2)
              for p in (False, True) if not (p and s == 2)]          # the entry takes a pass-through at stride 1 only (header)


@pytest.mark.parametrize("Cx,N,Nr,H,W,stride,with_pass", DWPW_CASES,
                         ids=[f"Cx{a}_N{c}_{d}x{e}_s{f}_{'pass' if g else 'nopass'}" for a, b, c, d, e, f, g in DWPW_CASES])
def test_shuffle_dwpw_exact(Cx, N, Nr, H, W, stride, with_pass):
    """the depthwise result never leaves the registers -> instrument 1 only; pads exact zeros, the pass-through half a bit copy."""
    B = 3
    rng = S.rng_of(43 + Cx + stride)
    assert _lib.load().mv_shuffle_dwpw_supported(Cx, N, stride, H, W, BF, BF) == 1
    x = S.int_tensor(rng, (B, H, W, Cx), 1)
    wdw = S.pm1_rows(rng, Cx, 9, 9).reshape(Cx, 3, 3, 1)
    ds, dh = S.int_scale(rng, Cx), S.int_tensor(rng, (Cx,), 2)
    wpw = np.zeros((N, Cx), np.float32)
    wpw[:Nr] = S.pm1_rows(rng, Nr, Cx, 4)
    ps, ph = np.zeros(N, np.float32), np.zeros(N, np.float32)
    ps[:Nr], ph[:Nr] = S.int_scale(rng, Nr), S.int_tensor(rng, (Nr,), 8)
    d, dm = S.conv_ref(x, wdw, ds, dh, None, 0, stride, 1, 1, Cx)
    Ho, Wo = d.shape[1], d.shape[2]
    ref, mag = S.gemm_ref(d.reshape(-1, Cx), wpw[:Nr], ps[:Nr], ph[:Nr], None, 1)
    S.prove_exact("dwpw d", d, dm, [wdw], stored=[x, wdw, wpw], min_nonzero=0.10)
    S.prove_exact("dwpw y", ref, mag, [wpw[:Nr]], hidden=[d])
    frag = torch.from_numpy(ops.dwpw_fragments(wpw)).to(torch.bfloat16).cuda()
    y_off = N if with_pass else 0
    pass_off = N - y_off
    y = _out((B, Ho, Wo, 2 * N))
    src, pass_args = None, (None, 0, 0, 0, 0, 0)
    if with_pass:
        src = _dev(S.bf(rng.standard_normal((B, Ho, Wo, 2 * N))))
        pass_args = (_p(src), 2 * N, N, Nr, pass_off, N)
    xd, wdd = _dev(x), _dev(wdw[..., 0].transpose(1, 2, 0))
    f = [_dev(a, "fp32") for a in (ds, dh, ps, ph)]
    _lib.call("mv_shuffle_dwpw_fwd", _p(xd), _p(wdd), _p(f[0]), _p(f[1]), _p(frag), _p(f[2]), _p(f[3]), _p(y), 2 * N, y_off, N, Nr, *pass_args, B, H, W, Cx, stride, BF, BF, _stream())
    kern = _lib.last_kernel()
    torch.cuda.synchronize()
    tag = f"shuffle_dwpw/Cx{Cx}_{H}x{W}_s{stride}_{'pass' if with_pass else 'nopass'}"
    assert bool((y[..., y_off + Nr:y_off + N] == 0).all()), f"{tag}: pads are not exact zeros"
    other = y[..., pass_off:pass_off + N]
    if with_pass:
        idx = torch.from_numpy(ops.shuffle_phys_index(2 * Nr, (Nr, N))[:Nr]).cuda()
        assert torch.equal(other[..., :Nr].view(torch.int16), src[..., idx].view(torch.int16)), f"{tag}: pass-through is not a bit copy"
        assert bool((other[..., Nr:] == 0).all()), tag
    else:
        assert bool((other == -7.0).all()), f"{tag}: the other half was touched"
    _verdict(tag, kern, f"shuffle_dwpw_s{stride}_m16", "int", [("y", _host(y[..., y_off:y_off + Nr]).reshape(-1, Nr), ref, None, 0, "bf16")])


# ================================================================================================ stems
def _nchw_ref(x_nchw, w_oihw, sc, sh, act, stride, pad):
    return S.conv_ref(x_nchw.transpose(0, 2, 3, 1), w_oihw.transpose(0, 2, 3, 1), sc, sh, None, act, stride, pad, 1)


STEM_CASES = [("7x7_s2_61x75", 1, 61, 75, 32, 7, 2, 3, 1, False, "stem_patch_mfma_f32in"), ("11x11_s4_67x67", 2, 67, 67, 64, 11, 4, 2, 1, False, "stem_patch_mfma_f32in"),
              ("patch16_tokens_64x64", 2, 64, 64, 768, 16, 16, 0, 0, True, "patch_embed_mfma_f32in")]


@pytest.mark.parametrize("mode", ["int", "gauss"])
@pytest.mark.parametrize("tag,N,H,W,K,R,stride,pad,act,tokens,expect", STEM_CASES, ids=[c[0] for c in STEM_CASES])
def test_stem_nchw(tag, N, H, W, K, R, stride, pad, act, tokens, expect, mode):
    _run_stem_nchw(tag, N, H, W, K, R, stride, pad, act, tokens, expect, mode)


@pytest.mark.parametrize("mode", ["int", "gauss"])
@pytest.mark.parametrize("tag,N,H,W,alexnet", [("resnet_75x93", 2, 75, 93, False), ("alexnet_67x67", 2, 67, 67, True)], ids=["resnet_75x93", "alexnet_67x67"])
def test_stem_pool(tag, N, H, W, alexnet, mode):
    """conv + BN + ReLU + max-pool in one launch.  The bf16 rounding is monotone, so max(round(v)) = round(max(v)): the reference is
    the max-pool of the float64 conv, and `mag` the max-pool of the conv's mag (an upper bound of every window member's)."""
    C, K = 3, 64
    R, st, pad, pp = (11, 4, 2, 0) if alexnet else (7, 2, 3, 1)
    rng = S.rng_of(52)
    assert _lib.load().mv_stem_conv_pool_supported(C, K, R, R, st, st, pad, pad, 3, 2, pp, 1, F32, BF, N * C * H * W)
    x = _x(mode, rng, (N, C, H, W), 2)
    w = _w(mode, rng, K, C * R * R, 16).reshape(K, C, R, R)
    sc = None if alexnet else _sc(mode, rng, K)
    sh = _sh(mode, rng, K)
    conv, cmag = _nchw_ref(x, w, sc, sh, 1, st, pad)
    pool = lambda a: torch.nn.functional.max_pool2d(torch.from_numpy(a).permute(0, 3, 1, 2), 3, 2, pp).permute(0, 2, 3, 1).numpy()
    ref, mag = pool(conv), pool(cmag)
    if mode == "int":
        S.prove_exact("stem_pool", ref, mag, [w], stored=[x, w], hidden=[conv])
    y = _out(ref.shape)
    xd, wd, scd, shd = _dev(x, "fp32"), _dev(w), (None if alexnet else _dev(sc, "fp32")), _dev(sh, "fp32")
    _lib.call("mv_stem_conv_pool_fwd", _p(xd), _p(wd), _p(scd), _p(shd), _p(y),
              N, C, H, W, K, R, R, st, st, pad, pad, 3, 2, pp, 1, F32, BF, _stream())
    kern = _lib.last_kernel()
    torch.cuda.synchronize()
    _verdict(f"stem_pool/{tag}/{mode}", kern, "stem_pool11_mfma_f32in" if alexnet else "stem_pool_mfma_f32in", mode, [("y", _host(y), ref, mag, C * R * R, "bf16")])
