"""`-m gpu`: exact +-1-row and per-element checks of the GEMM kernels that normalise their rows on the way in -- mv_ln_linear_fwd,
mv_ln_mlp_fwd, mv_ln_mlp_res_fwd, mv_ln_mlp_stream_fwd, mv_ln_mlp_stream_res_fwd -- and of the kernels whose LayerNorm follows the
accumulation or sits in the consumer's epilogue: mv_cnblock_dw_fwd (two exact cases, the normalize = 1 bound), mv_patch4_ln_fwd and
mv_linear_lnout_fwd -> mv_linear_lnin_fwd.  Instruments, derivations and case tables: tests/_strict_lngemm.py; the CPU proof that
they see each seeded defect: tests/test_strict_lngemm_host.py.

Every test names the kernel it must reach (`_lib.last_kernel()`; a call served by anything else fails), writes into a sentinel-filled
destination with a guard behind it, and prints its figures (`pytest -s`): exact -> the number of wrong elements; bound -> the worst
|got - ref| / bound, the violations, and the rounding bias where the project's rule applies.

Exact instrument (test_*_exact).  Facts from the source: the fragment is pack_bf2((x - mean) * rstd); gelu_tanh_pack2 is
x * rcp(1 + exp2(t)); for |x| >= 16 the result is x or -0 by the fp32 addition 1 + e = 1 (e < 2^-25) and by IEEE special values.
SUPPOSED (not in the source; a GPU that contradicts one shows as wrong elements at pre-activations of exactly 0 or at positive ones):
v_rcp_f32(1) = 1, v_rcp_f32(2) = 0.5, v_exp_f32(0) = 1.  -0 counts as equal to 0.

Shapes.  The entries' gates are M >= 8192 (ln_linear), 1024 (ln_mlp), 128 (ln_mlp_stream); below them the entry must refuse
(test_below_the_gate_is_refused), so the tail shapes sit right above: the gate itself (whole tiles), gate + 1, + 31 and + 33 rows
(a last tile of 1, 31 and 1 rows), and
the smallest 32 t + 5 at which one wave walks to a second tile of its strided list (t = 2048 for ln_linear: 256 blocks x 8 waves;
t = 3072 for ln_mlp: 256 x 12; t = 2048 with ln_mlp_waves=8, the kernel's prefetching path).  ln_mlp_stream runs one block per tile:
one tile, a ragged tail, and a third block.

Worst |got - ref| / bound per kernel over all its cases, measured on an MI355X, next to the CPU emulation's figure at its one case
(tests/_strict_lngemm.py).  No case violated its bound or differed in an exact test, the three supposed facts held, and no kernel
had to be changed:
    kernel                          MI355X   emulation        kernel                          MI355X   emulation
    stream1x1_ln_f32in_k96          0.588    0.482            ln_mlp96_f32stream              0.034    0.025
    stream1x1_ln_bf16in_k96         0.531    --               ln_mlp96_bf16stream             0.420    0.420
    stream1x1_ln_f32in_k192         0.425    --               ln_mlp96_res_f32in              0.025    0.025
    stream1x1_ln_bf16in_k192        0.446    0.389            ln_mlp96_res_bf16in             0.023    0.022
    ln_mlp_stream_c192_f32stream    0.012    0.011            ln_mlp_stream_c384_f32stream    0.005    0.005
    ln_mlp_stream_c192_res          0.012    0.011            ln_mlp_stream_c384_res          0.005    0.005
    cnblock_dw7_ln_f32in            0.986    0.986            cnblock_dw7_ln_bf16in           0.986    0.986
    swin_stem_ln_k96                0.006    0.005            swin_stem_ln_k128               0.005    0.005
    igemm8_bf16_256x256_dense_lnin  0.417    0.417            (the producer ..._lin_lnout_f32res: hi, lo, sum, mean, var all inside)
cnblock's 0.986 is the bf16 store's half ulp, which is nearly the whole of its bound: the accumulation and LayerNorm terms leave about
1.4 % of headroom, so a violation by a hair there is first to be read as another legitimate summation order, then as a bug.
"""
import numpy as np
import pytest
import torch

from eqxvision_amd import _lib
from tests import _strict as S
from tests import _strict_lngemm as G
from tests import _strict_norm as N
from tests._slices import GUARD, SENTINEL, _dest, _read
from tests._strict_gpu import DT, _dev, _Flags, _need_gpu, _p, _stream  # noqa: F401  (_need_gpu: the module fixture)

pytestmark = pytest.mark.gpu

F64 = np.float64
TT = {"bf16": torch.bfloat16, "fp32": torch.float32}
BF = _lib.BF16
assert G.SENTINEL == SENTINEL


def _take(y, M, C, tag):
    torch.cuda.synchronize()
    body, guard = _read(y, M, C)
    assert guard.numel() == GUARD and bool((guard == SENTINEL).all()), f"{tag}: guard behind the destination overwritten"
    return body.numpy().astype(F64)


def _exact(tag, kern, expect, got, ref):
    e = S.check_exact(got, ref)
    print(f"{tag} [{kern}]: exact {e['ok']}, wrong {e.get('nbad')} of {e.get('n')}")
    assert kern == expect, f"{tag}: served by {kern!r}, expected {expect!r}"
    assert e["ok"], f"{tag}: {e}"


def _bound(tag, kern, expect, got, ref, bound, out):
    a, b = N.judge(got, ref, bound, out)
    print(f"{tag} [{kern}]: worst |got-ref|/bound {a.get('worst', float('nan')):.3f} over {a.get('n')} elements, "
          f"violations {a.get('nviol')} | bias {b['bias']:+.4f} over {b['n_bias']}")
    assert kern == expect, f"{tag}: served by {kern!r}, expected {expect!r}"
    left = int(((got == SENTINEL) & (np.abs(np.asarray(ref) - SENTINEL) > bound)).sum())
    assert left == 0, f"{tag}: {left} sentinel values left inside the output"
    assert a["ok"], f"{tag} bound: {a}"
    assert b["ok"], f"{tag} bias: {b}"


# ================================================================================================ mv_ln_linear_fwd
def _ln_linear(tag, x, wf, bfold, M, K, N_, stream, act, flags):
    xd, wd, bd = _dev(np.array(x), stream), _dev(np.array(wf), "bf16"), _dev(np.array(bfold), "fp32")
    y = _dest(M, N_)
    with _Flags(flags):
        assert _lib.load().mv_ln_linear_supported(M, N_, K, DT[stream], BF) == 1, tag
        _lib.call("mv_ln_linear_fwd", _p(xd), _p(wd), _p(bd), _p(y), M, N_, K, G.EPS, act, DT[stream], BF, _stream())
        kern = _lib.last_kernel()
    return _take(y, M, N_, tag), kern


@pytest.mark.parametrize("act", [0, 1], ids=["none", "relu"])
@pytest.mark.parametrize("case", G.LINEAR_CASES, ids=G.linear_id)
def test_ln_linear_exact(case, act):
    """+-1 rows, W' = W diag(gamma) with W in {-1, 0, 1} and gamma in {1, 2}, b' = b + W beta in integers: bit equality."""
    M, K, N_, stream, flags = case
    x, wf, bfold, _, ref = G.linear_exact(M, K, N_, stream, act)
    tag = f"ln_linear/exact/{G.linear_id(case)}/act{act}"
    got, kern = _ln_linear(tag, x, wf, bfold, M, K, N_, stream, act, flags)
    _exact(tag, kern, G.linear_kernel(K, stream), got, ref)


@pytest.mark.parametrize("act", [0, 2], ids=["none", "gelu"])
@pytest.mark.parametrize("case", G.LINEAR_CASES, ids=G.linear_id)
def test_ln_linear_bound(case, act):
    """Gaussian rows (offset rows, one constant row) against float64 on the kernel's own operands: every element within the
    composed bound (LayerNorm bound through |W'|, the accumulation, GELU's Lipschitz constant and operations, the store)."""
    M, K, N_, stream, flags = case
    x, wf, bfold, _, ref, bound = G.linear_gauss(M, K, N_, stream, act)
    tag = f"ln_linear/bound/{G.linear_id(case)}/act{act}"
    got, kern = _ln_linear(tag, x, wf, bfold, M, K, N_, stream, act, flags)
    _bound(tag, kern, G.linear_kernel(K, stream), got, ref, bound, "bf16")


# ================================================================================================ mv_ln_mlp_fwd / mv_ln_mlp_res_fwd
def _ln_mlp(tag, x, res, w1, b1, w2, b2, M, C, stream, out, flags, streamed):
    Hd = 4 * C
    if streamed:
        w1, w2 = G.stream_fragments(np.asarray(w1), np.asarray(w2))
    xd, w1d, b1d = _dev(np.array(x), stream), _dev(np.array(w1), "bf16"), _dev(np.array(b1), "fp32")
    w2d, b2d = _dev(np.array(w2), "bf16"), _dev(np.array(b2), "fp32")
    rd = None if res is None else _dev(np.array(res), "fp32")
    y = _dest(M, C, TT[out])
    name = "mv_ln_mlp" + ("_stream" if streamed else "") + ("_res" if res is not None else "")
    with _Flags(flags):
        assert getattr(_lib.load(), name + "_supported")(M, C, Hd, DT[stream]) == 1, tag
        head = (_p(xd),) + (() if res is None else (_p(rd),))
        _lib.call(name + "_fwd", *head, _p(w1d), _p(b1d), _p(w2d), _p(b2d), _p(y), M, C, Hd, G.EPS, DT[stream], _stream())
        kern = _lib.last_kernel()
    return _take(y, M, C, tag), kern


@pytest.mark.parametrize("case", G.MLP96_CASES, ids=G.mlp96_id)
def test_ln_mlp_exact(case):
    """The whole chain in integers: +-1 fragments, fc1 in multiples of 16 (GELU is then an exact ReLU: module docstring, with the
    three supposed facts), fc2 in {-1, 0, 1}, integer biases and residual.  Bit equality; -0 equals 0."""
    M, stream, with_res, flags = case
    x, res, w1f, b1f, _, w2, b2, ref, out = G.mlp_exact(M, 96, stream, with_res)
    tag = "ln_mlp/exact/" + G.mlp96_id(case)
    got, kern = _ln_mlp(tag, x, res, w1f, b1f, w2, b2, M, 96, stream, out, flags, False)
    _exact(tag, kern, G.mlp96_kernel(stream, with_res), got, ref)


@pytest.mark.parametrize("case", G.MLP96_BOUND_CASES, ids=G.mlp96_id)
def test_ln_mlp_bound(case):
    """Gaussian rows against float64 on the kernel's operands, the bound composed through both GEMMs and the GELU (of the three
    second-tile shapes the fp32 stream's: their float64 references are the slowest of the module)."""
    M, stream, with_res, flags = case
    x, res, w1f, b1f, _, w2, b2, ref, bound, out = G.mlp_gauss(M, 96, stream, with_res)
    tag = "ln_mlp/bound/" + G.mlp96_id(case)
    got, kern = _ln_mlp(tag, x, res, w1f, b1f, w2, b2, M, 96, stream, out, flags, False)
    _bound(tag, kern, G.mlp96_kernel(stream, with_res), got, ref, bound, out)


# ================================================================================================ mv_ln_mlp_stream_fwd / _res_fwd
@pytest.mark.parametrize("case", G.STREAM_CASES, ids=G.stream_id)
def test_ln_mlp_stream_exact(case):
    M, C, with_res = case
    x, res, w1f, b1f, _, w2, b2, ref, out = G.mlp_exact(M, C, "fp32", with_res)
    tag = "ln_mlp_stream/exact/" + G.stream_id(case)
    got, kern = _ln_mlp(tag, x, res, w1f, b1f, w2, b2, M, C, "fp32", out, (), True)
    _exact(tag, kern, G.stream_kernel(C, with_res), got, ref)


@pytest.mark.parametrize("case", G.STREAM_CASES, ids=G.stream_id)
def test_ln_mlp_stream_midpoint_exact(case):
    """Rows whose normalised values sit just above a bf16 rounding midpoint (a variance over C - 1 moves them one ulp down, which the
    +-1 rows cannot show at C = 384), one channel per hidden unit, fc2 in {-1, 0, 1}: bit equality."""
    M, C, with_res = case
    x, res, w1f, b1f, w2, b2, ref = G.mlp_midpoint(M, C, with_res)
    tag = "ln_mlp_stream/midpoint/" + G.stream_id(case)
    got, kern = _ln_mlp(tag, x, res, w1f, b1f, w2, b2, M, C, "fp32", "fp32", (), True)
    _exact(tag, kern, G.stream_kernel(C, with_res), got, ref)


@pytest.mark.parametrize("case", G.STREAM_CASES, ids=G.stream_id)
def test_ln_mlp_stream_bound(case):
    M, C, with_res = case
    x, res, w1f, b1f, _, w2, b2, ref, bound, out = G.mlp_gauss(M, C, "fp32", with_res)
    tag = "ln_mlp_stream/bound/" + G.stream_id(case)
    got, kern = _ln_mlp(tag, x, res, w1f, b1f, w2, b2, M, C, "fp32", out, (), True)
    _bound(tag, kern, G.stream_kernel(C, with_res), got, ref, bound, out)


# ================================================================================================ mv_cnblock_dw_fwd: exact cases
def _cnblock(tag, x, w, bias, C, xdt, ydt, normalize):
    N_, H, W = G.cnb_shape(C)
    xd, wd = _dev(np.array(x), xdt), _dev(np.array(w), "bf16")
    bd = None if bias is None else _dev(np.array(bias), "fp32")
    y = _dest(N_ * H * W, C, TT[ydt])
    assert _lib.load().mv_cnblock_dw_supported(C, H, W, DT[xdt], DT[ydt], normalize) == 1, tag
    _lib.call("mv_cnblock_dw_fwd", _p(xd), _p(wd), _p(bd), _p(y), N_, H, W, C, G.EPS, normalize, DT[xdt], DT[ydt], _stream())
    kern = _lib.last_kernel()
    return _take(y, N_ * H * W, C, tag).reshape(N_, H, W, C), kern


@pytest.mark.parametrize("ydt", ["bf16", "fp32"])
@pytest.mark.parametrize("C,xdt", G.CNB_CASES)
def test_cnblock_dw_exact_integers(C, xdt, ydt):
    """normalize = 0: integer map and filters (a pattern per tap and per channel), integer bias, a width of TW + 5: bit equality."""
    x, w, bias, ref = G.cnb_exact(C)
    tag = f"cnblock/exact/C{C}/{xdt}/{ydt}"
    got, kern = _cnblock(tag, x, w, bias, C, xdt, ydt, 0)
    _exact(tag, kern, f"cnblock_dw7_{'f32in' if xdt == 'fp32' else 'bf16in'}" + ("_f32out" if ydt == "fp32" else ""), got, ref)


@pytest.mark.parametrize("C,xdt", G.CNB_CASES)
def test_cnblock_dw_ln_signs(C, xdt):
    """normalize = 1: x constant over the channels, w = sigma_c f[r][s]: the output is exactly sigma_c sign(f * x) at every pixel
    whose f * x is not zero (tests/_strict_lngemm.py: cnb_sign)."""
    x, w, ref, keep = G.cnb_sign(C)
    tag = f"cnblock/signs/C{C}/{xdt}"
    got, kern = _cnblock(tag, x, w, None, C, xdt, "bf16", 1)
    _exact(tag, kern, f"cnblock_dw7_ln_{'f32in' if xdt == 'fp32' else 'bf16in'}", got[keep], ref[keep])


@pytest.mark.parametrize("C,xdt", G.CNB_CASES)
def test_cnblock_dw_ln_bound(C, xdt):
    """normalize = 1 on a Gaussian map (one pixel of a constant window aside): the depthwise accumulation bound pushed through the
    LayerNorm's sensitivity, plus the LayerNorm's own bound (tests/_strict_lngemm.py: post_ln_bound).  Measured 0.986 of the bound: the
    bf16 store's half ulp is nearly all of it, so a failure by a hair is first a question of summation order, then of a bug."""
    x, w, bias, ref, bound = G.cnb_gauss(C, xdt)
    tag = f"cnblock/bound/C{C}/{xdt}"
    got, kern = _cnblock(tag, x, w, bias, C, xdt, "bf16", 1)
    _bound(tag, kern, f"cnblock_dw7_ln_{'f32in' if xdt == 'fp32' else 'bf16in'}", got, ref, bound, "bf16")


# ================================================================================================ mv_patch4_ln_fwd
@pytest.mark.parametrize("B,H,K,split", G.PATCH4_CASES)
def test_patch4_ln_bound(B, H, K, split):
    """The 4 x 4 / 4 patch GEMM (hi + lo filter terms) with the LayerNorm behind it, fp32 output: the accumulation bound pushed through
    the LayerNorm's sensitivity plus the LayerNorm's own bound; one tile, ragged tiles, K = 96 and 128, both filter forms."""
    x, hi, lo, b, g, be, ref, bound = G.patch4_gauss(B, H, K, split)
    M = ref.shape[0]
    xd, hid, lod = _dev(np.array(x), "fp32"), _dev(np.array(hi), "bf16"), _dev(np.array(lo), "bf16")
    bd, gd, bed = _dev(np.array(b), "fp32"), _dev(np.array(g), "fp32"), _dev(np.array(be), "fp32")
    y = _dest(M, K, torch.float32)
    tag = f"patch4_ln/bound/B{B}_H{H}_K{K}_split{int(split)}"
    assert _lib.load().mv_patch4_ln_supported(3, H, H, K, DT["fp32"]) == 1, tag
    _lib.call("mv_patch4_ln_fwd", _p(xd), _p(hid), _p(lod) if split else None, _p(bd), _p(gd), _p(bed), _p(y), B, 3, H, H, K, G.EPS,
              DT["fp32"], _stream())
    kern = _lib.last_kernel()
    _bound(tag, kern, f"swin_stem_ln_k{K}", _take(y, M, K, tag), ref, bound, "fp32")


# ================================================================================================ mv_linear_lnout_fwd -> mv_linear_lnin_fwd
@pytest.mark.parametrize("case", G.LNFOLD_CASES, ids=G.lnfold_id)
def test_lnfold_pair(case):
    """Producer (fp32 rows -> planes + statistics): hi a correct bf16 rounding, |lo| within half an ulp of hi, hi + lo and the
    Chan-merged statistics against float64, every element / row.  Consumer on the producer's OWN planes and table: every element
    within lnin_ref_bound (operand rounding of hi, statistics, accumulation on the un-normalised rows), plus the bias rule."""
    M, D, Kp, N2, act, row_mean = case
    x, w, b, res, wf, cs, bfold = G.lnfold_data(*case)
    y_ref, e_y = G.lnout_ref(*case)
    tag = "lnfold/" + G.lnfold_id(case)
    L = _lib.load()
    assert L.mv_linear_lnout_supported(M, D, Kp, BF) == 1 and L.mv_linear_lnin_supported(M, N2, D, 0, 0, BF) == 1, tag
    xd, wd, bd, rd = _dev(np.array(x)), _dev(np.array(w)), _dev(np.array(b), "fp32"), _dev(np.array(res), "fp32")
    P = -(-D // 256)
    hi, lo = _dest(M, D), _dest(M, D)
    st = torch.full((P * M * 2 + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    _lib.call("mv_linear_lnout_fwd", _p(xd), _p(wd), _p(bd), _p(rd), None, _p(hi), _p(lo), _p(st), M, D, Kp, BF, _stream())
    k1 = _lib.last_kernel()
    hh, ll = _take(hi, M, D, tag + "/hi"), _take(lo, M, D, tag + "/lo")
    sth = st.cpu().numpy().astype(F64)
    assert (sth[P * M * 2:] == SENTINEL).all(), f"{tag}: guard behind the statistics overwritten"
    info = G.check_lnout(hh, ll, sth[:P * M * 2].reshape(P, M, 2), y_ref, e_y)
    print(f"{tag} [{k1}]: " + ", ".join(f"{k} ok {v['ok']} worst {v['worst']:.4g}" for k, v in info.items()))
    assert k1 == "igemm8_bf16_256x256_lin_lnout_f32res", k1
    for k, v in info.items():
        assert v["ok"], f"{tag} {k}: {v}"
    ref, bound = G.lnin_ref_bound(hh, ll, wf, cs, bfold, act)
    wfd, csd, bfd = _dev(np.array(wf)), _dev(np.array(cs), "fp32"), _dev(np.array(bfold), "fp32")
    y = _dest(M, N2)
    _lib.call("mv_linear_lnin_fwd", _p(hi), _p(st), _p(wfd), _p(csd), _p(bfd), _p(y), M, N2, D, G.LNFOLD_EPS, act, 0, 0, BF, _stream())
    k2 = _lib.last_kernel()
    _bound(tag + "/lnin", k2, "igemm8_bf16_256x256_dense_lnin", _take(y, M, N2, tag + "/y"), ref, bound, "bf16")


# ================================================================================================ the gates
@pytest.mark.parametrize("M", [1, 31, 33, G.MLP_MIN_M - 1])
def test_below_the_gate_is_refused(M):
    """Rows below an entry's gate are not served by these kernels: _supported says 0 and the call fails loudly (MV_E_UNSUPPORTED)
    with the destination untouched -- never another kernel in silence.  The same for ln_linear below 8192 and ln_mlp_stream below 128."""
    L = _lib.load()
    x = _dev(np.zeros((G.LINEAR_MIN_M, 96), np.float32), "fp32")
    w1, w2 = _dev(np.zeros((384, 96), np.float32), "bf16"), _dev(np.zeros((96, 384), np.float32), "bf16")
    b = _dev(np.zeros(384, np.float32), "fp32")
    y = _dest(G.LINEAR_MIN_M, 96, torch.float32)
    calls = [("mv_ln_mlp_fwd", (_p(x), _p(w1), _p(b), _p(w2), _p(b), _p(y), M, 96, 384, G.EPS, DT["fp32"], _stream()))]
    assert L.mv_ln_mlp_supported(M, 96, 384, DT["fp32"]) == 0 and L.mv_ln_mlp_res_supported(M, 96, 384, DT["fp32"]) == 0
    assert L.mv_ln_linear_supported(min(M * 8, G.LINEAR_MIN_M - 1), 384, 96, DT["fp32"], BF) == 0
    calls.append(("mv_ln_linear_fwd", (_p(x), _p(w1), _p(b), _p(y), min(M * 8, G.LINEAR_MIN_M - 1), 384, 96, G.EPS, 0, DT["fp32"], BF,
                                       _stream())))
    if M < G.STREAM_MIN_M:
        assert L.mv_ln_mlp_stream_supported(M, 192, 768, DT["fp32"]) == 0
    for name, args in calls:
        with pytest.raises(_lib.MVError, match="unsupported"):
            _lib.call(name, *args)
    torch.cuda.synchronize()
    assert bool((y == SENTINEL).all())
