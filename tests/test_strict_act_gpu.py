"""`-m gpu`: the activations fused into the conv / GEMM epilogues, and mv_se_scale_fwd, under the two strict instruments
(tests/_strict.py, "fused activations"; runners in tests/_strict_gpu.py; CPU proofs in tests/test_strict_act_host.py).

Every (kernel, activation) pair the library implements runs mode "int" (bit equality on the activation's lattice) and mode
"gauss" (S.act_bound on every element, the rounding bias where it applies) on ONE shape: the smallest ragged row the tables of
tests/test_strict_gpu.py use for that kernel.  Each case pins `_lib.last_kernel()` and prints the verdict (`pytest -s`).

gelu_tanh (2):  igemm.hip's three 128-row instances and the odd-C kernel; igemm8 at its three tiles with a bf16 output (the packed
gelu_tanh_pack2 path) and an fp32 output (the scalar path), and its split-K launch (mode int only, as test_splitk_linear_exact);
igemm2 tiles 1 and 3, bf16 and fp32 output; conv3x3c64_halo; stream1x1 (three reductions); skinny_linear_mfma; the three fp32
compute kernels; conv_generic; fc_stream_bf16; the five depthwise kernels; the three epilogues of stem.hip.
hard_swish, hard_sigmoid, sigmoid, silu (3 - 6):  stream1x1; the `_act` route of igemm.hip; the odd-C kernel (route.h gives it no
`_act` suffix); conv_generic, conv_f32_mfma, conv_f32_lds_mfma; the depthwise kernels; the stems; fc_stream_bf16 (its entry takes them).

Left out, with the reason:
  * mv_linear_fwd refuses 3 - 6 (MV_CHECK_FUSED_ACT): asserted once, test_entries_refuse_unfused_act.  The stream1x1, odd-C and
    `no_stream` rows therefore go through mv_conv2d_nhwc_fwd as 1 x 1 convolutions for 3 - 6 (gelu_tanh keeps mv_linear_fwd);
    skinny_linear_mfma and skinny_linear_f32_mfma are reached from mv_linear_fwd's rule only for none / ReLU / gelu_tanh.
  * mv_stem_conv_pool_fwd refuses 3 - 6 the same way and supports ReLU alone (stem_pool.hip): its epilogues have no other branch.
  * stem.hip: all three epilogues are reachable through mv_conv2d_nchw_fwd with every activation -- stem_kernel
    (`stem_conv_mfma_f32in`: a 3 x 3 stride-2 stem, S <= 4 keeps it off the patch kernel), stem_patch_kernel
    (`stem_patch_mfma_f32in`: 7 x 7 stride 2) and patch_embed_kernel (`patch_embed_mfma_f32in`: 16 x 16 patches with token rows;
    the position rows are added before the activation).
  * igemm8, igemm2, conv3x3c64_halo: route.h sends 3 - 6 to igemm.hip or stream1x1 before it asks them.

mv_se_scale_fwd (`se_scale_fused`), N = 3 images, against the float64 reference of the header's definition (S.se_ref):
    (C, S, HW)        reaches
    (16, 4, 1)        one pixel: pl = 512 pixel lanes, 511 of them idle
    (72, 19, 5)       cpb = 9 leaves 7 idle threads; HW < pl; S > 16: a second trip of the wave loop; S % 4 = 3: fc2's scalar tail
    (1032, 6, 67)     a second channel group with cpb = 1, pl = 1024; C > 1024: a second trip of the fc2 thread loop
    (96, 33, 343)     the 4-way unrolled pixel loop and its tail (pl = 85, HW = 4 * 85 + 3)
with (silu, sigmoid), (relu, hard_sigmoid), (none, none), each with and without b1 / b2.  3 C < 4096 outputs: no bias verdict.

Supposed of the hardware (tests/_strict.py): v_exp_f32(+-0) = 1, v_rcp_f32(1) = 1, v_rcp_f32(2) = 0.5, exp2 below -128 is below 2^-25,
exp2 above 128 is +inf.

Measured on an MI355X (records, not thresholds: the thresholds are ratio <= 1 on every element and |bias| <= S.BIAS_LIMIT).  All
274 cases pass; every lattice case is bit-equal, pre-activation 0 of sigmoid / hard_sigmoid included (the suppositions hold).
Worst |got - ref| / bound and worst |bias| per kernel, over its activations (gelu_tanh | hard_swish, hard_sigmoid, sigmoid, silu):
    igemm_bf16_128x128_conv / 128x64_conv / igemm8 (three tiles) bf16 out   0.945, bias 0.002 |  -
    igemm_bf16_128x128_dense, igemm8 *_conv_f32out (fp32 out)              0.003            |  -
    igemm2_bf16_256x64_conv / 256x256_conv                                 0.948            |  -
    conv3x3c64_halo                                                        0.944            |  -
    skinny_linear_mfma / skinny_linear_f32_mfma                            0.988 / 0.006    |  -
    igemm_bf16_128x128_conv_act / 128x64_conv_act / 128x128_dense_act      -                |  0.957 / 0.883 / 0.997, bias 0.011
    igemm_bf16_128x64_dense_oddc                                           0.973            |  0.988
    stream1x1 k64 / k16 / k128 (fp32 out)                                  0.994 / 0.998 / 0.006 | 0.997 / 1.000 / 0.009, bias 0.008
    conv_generic                                                           0.945            |  0.957, bias 0.012
    conv_f32_mfma / conv_f32_lds_mfma                                      0.005 / 0.002    |  0.006 / 0.002
    fc_stream_bf16                                                         0.876            |  0.882, bias 0.008
    dwconv (five kernels)                                                  0.997            |  1.000 as printed (no violation), bias 0.007
    stem_conv / stem_patch / patch_embed _mfma_f32in                       0.995 / 0.985 / 0.904 | 0.999 / 0.991 / 0.930, bias 0.017
    se_scale_fused                                                         0.992 (silu, sigmoid), 0.999 (relu, hard_sigmoid), 0.982 (none, none)
A bf16 output puts the ratio near 1 by construction (the store's half ulp is the bound's main term); the CPU emulation of
tests/test_strict_act_host.py gives 0.991 - 0.997 (bf16), 0.008 - 0.017 (fp32) and bias <= 0.007 on its 520 x 64 x 72 GEMM, and
0.907 - 0.999 for se_scale -- the same figures as the kernel on the se_scale cases, whose order of operations it follows.
Wall time of the module on the MI355X: 8.5 s (274 cases; the slowest 0.26 s).
"""
import numpy as np
import pytest
import torch

from eqxvision_amd import _lib
from tests import _strict as S
from tests._strict_gpu import (BF, _dev, _Flags, _guard_ok, _host, _need_gpu, _out_guarded, _p, _run_conv, _run_dwconv,  # noqa: F401
                               _run_fc_stream, _run_stem_nchw, _stream, _verdict)
from tests.test_strict_gpu import _BIG, CONV_SHAPES, DW_CASES, F32_CASES

pytestmark = pytest.mark.gpu

GELU = 2
UNFUSED = (3, 4, 5, 6)                    # hard_swish, hard_sigmoid, sigmoid, silu
M_STREAM = 8192 + 37


def _lin(M, Kr, N):
    return (1, M, 1, Kr, N, 1, 1, 0, 1)


def _row(table, name):
    sh, _, res, out = table[name]
    return dict(shape=sh, res=res, out=out)


# tag -> (expected kernel, _run_conv keywords); `modes` where not both
CONV_GELU = {
    "igemm128x128_conv": ("igemm_bf16_128x128_conv", dict(_row(CONV_SHAPES, "3x3_64_72"))),
    "igemm128x64_conv": ("igemm_bf16_128x64_conv", dict(_row(CONV_SHAPES, "3x3_64_72"), flags=("igemm_tile=2",))),
    "igemm128x128_dense": ("igemm_bf16_128x128_dense", dict(_row(CONV_SHAPES, "1x1_192_264_res_f32out"))),
    "oddc_17x144x64": ("igemm_bf16_128x64_dense_oddc", dict(shape=_lin(17, 144, 64), linear=True)),
    **{f"igemm8={f}_bf16": (f"igemm8_bf16_{t}_conv", dict(_row(CONV_SHAPES, "3x3_64_72"), flags=(f"igemm8={f}",)))
       for f, t in ((2, "256x256"), (3, "128x256"), (4, "256x128"))},
    **{f"igemm8={f}_f32out": (f"igemm8_bf16_{t}_conv_f32out", dict(_row(CONV_SHAPES, "3x3_64_72_res_f32out"), flags=(f"igemm8={f}",)))
       for f, t in ((2, "256x256"), (3, "128x256"), (4, "256x128"))},
    "igemm8_splitk": ("igemm8_bf16_128x256_dense_splitk", dict(shape=_lin(3136, 832, 512), res=True, linear=True, splitk=True,
                                                               flags=("splitk_min_nk=12",), modes=("int",))),
    **{f"igemm2_tile={t}_{o}": (f"igemm2_bf16_{tile}_conv", dict(_row(_BIG, s), flags=(f"igemm2_tile={t}",)))
       for t, tile in ((1, "256x64"), (3, "256x256")) for o, s in (("bf16", "3x3_64_72"), ("f32out", "3x3_64_72_res_f32out"))},
    "conv3x3c64_halo": ("conv3x3c64_halo", dict(shape=(69, 12, 10, 64, 64, 3, 1, 1, 1))),
    "stream_64_256_res": ("stream1x1_bf16_bn128_k64", dict(shape=_lin(M_STREAM, 64, 256), res=True, linear=True)),
    "stream_16_96": ("stream1x1_bf16_bn128_k16", dict(shape=_lin(M_STREAM, 16, 96), linear=True, nnz=8)),
    "stream_128_200_f32out": ("stream1x1_bf16_bn128_k128", dict(shape=_lin(M_STREAM, 128, 200), res=True, out="fp32", linear=True)),
    "skinny_33x64x40": ("skinny_linear_mfma", dict(shape=_lin(33, 64, 40), linear=True)),
    **{f"f32/{tag}": (expect, dict(shape=sh, res=res, dtype="fp32", out="fp32", linear=linear, nnz=nnz))
       for tag, sh, _, res, linear, nnz, expect in F32_CASES},
    "conv_generic": ("conv_generic", dict(_row(CONV_SHAPES, "3x3_64_72"), flags=("force_generic",))),
}
# 3 - 6: everything through mv_conv2d_nhwc_fwd (mv_linear_fwd refuses them)
CONV_UNFUSED = {
    "stream_64_256_res": ("stream1x1_bf16_bn128_k64", dict(shape=_lin(M_STREAM, 64, 256), res=True)),
    "stream_16_96": ("stream1x1_bf16_bn128_k16", dict(shape=_lin(M_STREAM, 16, 96), nnz=8)),
    "stream_128_200_f32out": ("stream1x1_bf16_bn128_k128", dict(shape=_lin(M_STREAM, 128, 200), res=True, out="fp32")),
    "act_3x3_64_72": ("igemm_bf16_128x128_conv_act", dict(_row(CONV_SHAPES, "3x3_64_72"))),
    "act_3x3_s2_128_64_res": ("igemm_bf16_128x64_conv_act", dict(_row(CONV_SHAPES, "3x3_s2_128_64_res"))),
    "act_1x1_192_264_res_f32out": ("igemm_bf16_128x128_dense_act", dict(_row(CONV_SHAPES, "1x1_192_264_res_f32out"))),
    "act_64_256_no_stream": ("igemm_bf16_128x128_dense_act", dict(shape=_lin(M_STREAM, 64, 256), res=True, flags=("no_stream",))),
    "oddc_17x144x64": ("igemm_bf16_128x64_dense_oddc", dict(shape=_lin(17, 144, 64))),
    "conv_generic": ("conv_generic", dict(_row(CONV_SHAPES, "3x3_64_72"), flags=("force_generic",))),
    **{f"f32/{tag}": (expect, dict(shape=sh, res=res, dtype="fp32", out="fp32", nnz=nnz))
       for tag, sh, _, res, linear, nnz, expect in F32_CASES if not linear},
}
ALL_ACTS = (GELU,) + UNFUSED
# split-K: instrument 1 only (equality holds whatever the hand-over order) -- its row names its modes
CONV_CASES = [(f"{tag}/{S.ACT_NAMES[a]}/{mode}", a, expect, kw, mode)
              for table, acts in ((CONV_GELU, (GELU,)), (CONV_UNFUSED, UNFUSED)) for tag, (expect, kw) in table.items() for a in acts
              for mode in kw.get("modes", ("int", "gauss"))]


@pytest.mark.parametrize("tag,act,expect,kw,mode", CONV_CASES, ids=[c[0] for c in CONV_CASES])
def test_conv_act(tag, act, expect, kw, mode):
    kw = {k: v for k, v in kw.items() if k not in ("shape", "modes")} | {"shape": kw["shape"]}
    _run_conv(f"act/{tag}", mode, kw.pop("shape"), expect, act=act, seed=61, **kw)


@pytest.mark.parametrize("mode", ["int", "gauss"])
@pytest.mark.parametrize("act", ALL_ACTS, ids=[S.ACT_NAMES[a] for a in ALL_ACTS])
def test_fc_stream_act(act, mode):
    _run_fc_stream(3, 1024, 4096, True, "bf16", mode, act=act)


@pytest.mark.parametrize("mode", ["int", "gauss"])
@pytest.mark.parametrize("act", ALL_ACTS, ids=[S.ACT_NAMES[a] for a in ALL_ACTS])
@pytest.mark.parametrize("tag,N,H,W,C,R,stride,flag,expect", DW_CASES, ids=[c[0] for c in DW_CASES])
def test_dwconv_act(tag, N, H, W, C, R, stride, flag, expect, act, mode):
    _run_dwconv(f"{tag}/{S.ACT_NAMES[act]}", N, H, W, C, R, stride, flag, expect, mode, act=act)


# mv_conv2d_nchw_fwd: (tag, N, H, W, K, R, stride, pad, tokens, kernel) -- one row per epilogue of stem.hip
STEM_ACT_CASES = [("3x3_s2_33x35_k24", 2, 33, 35, 24, 3, 2, 1, False, "stem_conv_mfma_f32in"),
                  ("7x7_s2_61x75", 1, 61, 75, 32, 7, 2, 3, False, "stem_patch_mfma_f32in"),
                  ("patch16_tokens_64x64", 2, 64, 64, 768, 16, 16, 0, True, "patch_embed_mfma_f32in")]


@pytest.mark.parametrize("mode", ["int", "gauss"])
@pytest.mark.parametrize("act", ALL_ACTS, ids=[S.ACT_NAMES[a] for a in ALL_ACTS])
@pytest.mark.parametrize("tag,N,H,W,K,R,stride,pad,tokens,expect", STEM_ACT_CASES, ids=[c[0] for c in STEM_ACT_CASES])
def test_stem_act(tag, N, H, W, K, R, stride, pad, tokens, expect, act, mode):
    _run_stem_nchw(f"{tag}/{S.ACT_NAMES[act]}", N, H, W, K, R, stride, pad, act, tokens, expect, mode)


def test_entries_refuse_unfused_act():
    """MV_CHECK_FUSED_ACT: mv_linear_fwd and mv_stem_conv_pool_fwd answer MV_E_INVALID (-1) to 3 - 6 before they look at anything
    else; nothing is launched (the destinations keep the sentinel)."""
    lib = _lib.load()
    x, w = _dev(np.zeros((8, 64), np.float32)), _dev(np.zeros((64, 64), np.float32))
    buf, y = _out_guarded((8, 64))
    img = _dev(np.zeros((1, 3, 32, 32), np.float32), "fp32")
    for act in UNFUSED:
        assert lib.mv_linear_fwd(_p(x), _p(w), None, None, None, _p(y), 8, 64, 64, act, BF, BF, _stream()) == -1
        assert lib.mv_stem_conv_pool_fwd(_p(img), _p(w), None, None, _p(y), 1, 3, 32, 32, 64, 7, 7, 2, 2, 3, 3, 3, 2, 1, act, _lib.F32, BF, _stream()) == -1
    torch.cuda.synchronize()
    assert bool((buf == S.SENTINEL).all().item())


# ================================================================================================ mv_se_scale_fwd
SE_CASES = [(C, Sq, HW, a1, a2, bias) for (C, Sq, HW) in S.SE_SHAPES for (a1, a2) in S.SE_ACTS for bias in (True, False)]


@pytest.mark.parametrize("mode", ["int", "gauss"])
@pytest.mark.parametrize("C,Sq,HW,a1,a2,bias", SE_CASES, ids=[f"{c[0]}_{c[1]}_{c[2]}_{c[3]}_{c[4]}_{'bias' if c[5] else 'nobias'}" for c in SE_CASES])
def test_se_scale(C, Sq, HW, a1, a2, bias, mode):
    assert C * Sq <= 65536 and _lib.load().mv_se_scale_supported(C, Sq, BF)
    x, w1, b1, w2, b2 = S.se_data(mode, C, Sq, HW, a1, a2, bias)
    if mode == "int":
        ref, bound = S.se_prove_exact("se_scale", x, w1, b1, w2, b2, a1, a2), None
    else:
        f = S.se_ref(x, w1, b1, w2, b2, a1, a2)
        ref, bound = f["ref"], f["bound"]
    xd, w1d, w2d = _dev(x), _dev(w1), _dev(np.ascontiguousarray(w2.T))                 # w2 handed over transposed (header)
    b1d, b2d = (None if b1 is None else _dev(b1, "fp32")), (None if b2 is None else _dev(b2, "fp32"))
    buf, y = _out_guarded((S.SE_N, C))
    _lib.call("mv_se_scale_fwd", _p(xd), _p(w1d), _p(b1d), _p(w2d), _p(b2d), _p(y), S.SE_N, HW, C, Sq, S.ACT_CODES[a1], S.ACT_CODES[a2], BF, _stream())
    kern = _lib.last_kernel()
    torch.cuda.synchronize()
    assert _guard_ok(buf), "se_scale: guard band behind the scale vector touched"
    _verdict(f"se_scale/{C}_{Sq}_{HW}/{a1}+{a2}/{'bias' if bias else 'nobias'}/{mode}", kern, "se_scale_fused", mode,
             [("scale", _host(y), ref, None, 0, "bf16", bound)])
