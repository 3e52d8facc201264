"""`-m gpu`: the kernels on the entry path into the GEMM cores under the two strict instruments -- the fp32-input image entries on
ROUNDING-VISIBLE images, the bf16-image / fp32-output / split-weight / generic-fallback forms of the NCHW entry, mv_linear_split_fwd,
the head-major stores of mv_linear_heads_fwd and mv_linear_lnin_fwd, and mv_vit_cls_pos_fwd.  Constructions, references, bounds:
tests/_strict_entry.py; the CPU proof that the instruments see each seeded defect: tests/test_strict_entry_host.py.

Every launch writes into a sentinel-filled destination with a guard band behind it, names the kernel it must reach
(`_lib.last_kernel()`), and prints its figures (`pytest -s`).  Rows a kernel must not write (the class row in token mode, rows 1 ..
of mv_vit_cls_pos_fwd) must keep the sentinel; a refused call must leave the whole destination untouched.

Measured on an MI355X (records, not thresholds: the thresholds are equality, ratio <= 1 on every element and |bias| <= S.BIAS_LIMIT).
All 139 cases pass, every exact case with 0 wrong elements, and no kernel had to be changed.  Worst |got - ref| / bound and worst
|bias| per kernel over its Gaussian cases (a bf16 output puts the ratio near 1 by construction: the store's half ulp is the bound's
main term), and the number of exact cases:
    kernel                                   ratio   |bias|   exact cases
    stem_conv_mfma_f32in                     --      --       1 (visible)
    stem_patch_mfma_f32in                    --      --       1 (visible)
    patch_embed_mfma_f32in                   --      --       1 (visible)
    stem_pool_mfma_f32in / stem_pool11_..    --      --       1 / 1 (visible)
    stem_conv_mfma_bf16in                    0.997   0.0012   1
    stem_patch_mfma_bf16in                   0.984   0.0017   1
    patch_embed_mfma_bf16in                  0.882   0.0004   1
    patch_embed_mfma_f32in_f32out            0.001   --       4 (1 visible)
    patch_embed_mfma_bf16in_f32out           0.001   --       3
    stem_conv_mfma_f32in_w2                  0.995   0.0028   4 (2 visible, 2 dyadic)
    stem_conv_mfma_bf16in_w2                 0.995   0.0028   2 (dyadic)
    conv_generic (token mode)                0.882   0.0005   1
    igemm8_dual_bf16_128x256 [_f32out]       0.991   0.0014   [0.009; 12 exact + 1 split-K]
    igemm8_dual_bf16_256x128 [_f32out]       0.982   0.0006   [0.007; 12 exact]
    igemm8_dual_bf16_256x256 [_f32out]       0.977   0.0001   [0.005; 4 exact]
    igemm8_bf16_{128x256,256x128,256x256}_dense, igemm8_bf16_256x256_lin, igemm2_bf16_256x{64,128,256}_dense (head-major)
                                             0.976   0.0003   3 each (tokens 197 / 50 / 256)
    igemm8_bf16_256x256_dense_lnin           0.429   0.0032   head-major == permuted token-major: 0 of 12 229 760 elements differ
    vit_cls_pos                              0.999   --       fp32: bit-equal to the one fp32 add
Wall time of the module on the MI355X: 6.3 s (the slowest case 0.8 s).
"""
import numpy as np
import pytest
import torch

from eqxvision_amd import _lib
from tests import _strict as S
from tests import _strict_entry as E
from tests import _strict_lngemm as G
from tests import _strict_norm as N_
from tests._strict_gpu import BF, DT, F32, _dev, _Flags, _guard_ok, _host, _need_gpu, _out_guarded, _p, _stream, _verdict  # noqa: F401

pytestmark = pytest.mark.gpu


def _opt(a, dtype="fp32"):
    return None if a is None else _dev(np.array(a), dtype)


def _refused(tag, name, args, buf):
    with pytest.raises(_lib.MVError, match="unsupported"):
        _lib.call(name, *args)
    torch.cuda.synchronize()
    assert bool((buf == S.SENTINEL).all().item()), f"{tag}: a refused call wrote to the destination"


# ================================================================================================ the NCHW entries
def _run_nchw(d, entry, expect, flags=()):
    """entry: "fwd" (mv_conv2d_nchw_fwd), "f32out", "split".  The verdict is taken on the rows the kernel owns; the class row of
    every image must still hold the sentinel."""
    N, C, H, W, K, R, st, pad, T, P = (d[k] for k in ("N", "C", "H", "W", "K", "R", "stride", "pad", "T", "P"))
    xd, hid, lod = _dev(np.array(d["x"]), d["xdtype"]), _dev(np.array(d["hi"])), _opt(d["lo"], "bf16")
    scd, shd, posd = _opt(d["scale"]), _opt(d["shift"]), _opt(d["pos"])
    buf, y = _out_guarded((N, T or P, K), d["out"])
    targs = (T, 1 if T else 0, _p(posd))
    geo = (N, C, H, W, K, R, R, st, st, pad, pad)
    tag = f"{entry}/{d['kind']}/{d['tag']}/{d['xdtype']}/{d['out']}/{d['mode']}"
    with _Flags(flags):
        if entry == "fwd":
            _lib.call("mv_conv2d_nchw_fwd", _p(xd), _p(hid), _p(scd), _p(shd), _p(y), *geo, 0, DT[d["xdtype"]], DT[d["out"]], *targs, _stream())
        elif entry == "f32out":
            assert _lib.load().mv_conv2d_nchw_f32out_supported(C, H, W, K, R, R, st, st, pad, pad, DT[d["xdtype"]]) == 1, tag
            _lib.call("mv_conv2d_nchw_f32out_fwd", _p(xd), _p(hid), _p(scd), _p(shd), _p(y), *geo, 0, DT[d["xdtype"]], *targs, _stream())
        else:
            _lib.call("mv_conv2d_nchw_split_fwd", _p(xd), _p(hid), _p(lod), _p(scd), _p(shd), _p(y), *geo, 0, DT[d["xdtype"]], DT[d["out"]], _stream())
        kern = _lib.last_kernel()
    torch.cuda.synchronize()
    assert _guard_ok(buf), f"{tag}: guard band behind y touched"
    got = _host(y)
    if T:
        assert bool((got[:, 0] == S.SENTINEL).all()), f"{tag}: the class row was written"
        got = got[:, 1:]
    _verdict(tag, kern, expect, "int" if d["exact"] else "gauss", [("y", got, d["ref"], d["mag"], d["kred"], d["out"])])


def _xin(xd):
    return "f32in" if xd == "fp32" else "bf16in"


@pytest.mark.parametrize("g", E.STEM_GEOMS, ids=E.geom_id)
def test_visible_stem(g):
    """A: fp32 pixels that are no bf16 values, 40 % exact ties; the result must EQUAL the reference on the RNE image."""
    _run_nchw(E.nchw_case("plain", "visible", *g, "fp32", "bf16"), "fwd", E.STEM_KERNELS[g[0]] + "_f32in")


def test_visible_f32out():
    _run_nchw(E.nchw_case("plain", "visible", *E.F32OUT_GEOMS[0], "fp32", "fp32"), "f32out", "patch_embed_mfma_f32in_f32out")


@pytest.mark.parametrize("g", E.SPLIT_GEOMS, ids=E.geom_id)
def test_visible_split(g):
    _run_nchw(E.nchw_case("split", "visible", *g, "fp32", "bf16"), "split", "stem_conv_mfma_f32in_w2")


@pytest.mark.parametrize("g", E.POOL_GEOMS, ids=E.geom_id)
def test_visible_stem_pool(g):
    tag, N, H, W, R, st, pad, pp, with_scale, expect = g
    p = E.pool_case(tag, N, H, W, R, st, pad, pp, with_scale)
    assert _lib.load().mv_stem_conv_pool_supported(3, 64, R, R, st, st, pad, pad, 3, 2, pp, 1, F32, BF, N * 3 * H * W)
    xd, wd, scd, shd = _dev(np.array(p["x"]), "fp32"), _dev(np.array(p["w"])), _opt(p["scale"]), _opt(p["shift"])
    buf, y = _out_guarded(p["ref"].shape)
    _lib.call("mv_stem_conv_pool_fwd", _p(xd), _p(wd), _p(scd), _p(shd), _p(y), N, 3, H, W, 64, R, R, st, st, pad, pad, 3, 2, pp, 1, F32, BF, _stream())
    kern = _lib.last_kernel()
    torch.cuda.synchronize()
    assert _guard_ok(buf), f"stem_pool/{tag}: guard band behind y touched"
    _verdict(f"visible/stem_pool/{tag}", kern, expect, "int", [("y", _host(y), p["ref"], p["mag"], 3 * R * R, "bf16")])


@pytest.mark.parametrize("mode", ["int", "gauss"])
@pytest.mark.parametrize("g", E.STEM_GEOMS, ids=E.geom_id)
def test_stem_bf16_image(g, mode):
    """B: the bf16-image instances of the three stem kernels."""
    _run_nchw(E.nchw_case("plain", mode, *g, "bf16", "bf16"), "fwd", E.STEM_KERNELS[g[0]] + "_bf16in")


@pytest.mark.parametrize("mode", ["int", "gauss"])
@pytest.mark.parametrize("xd", ["fp32", "bf16"])
@pytest.mark.parametrize("g", E.F32OUT_GEOMS, ids=E.geom_id)
def test_f32out(g, xd, mode):
    """fp32 token rows: a ragged row tile, a ragged channel tile (K = 200), remainder rows (H = 70), token mode and dense rows."""
    _run_nchw(E.nchw_case("plain", mode, *g, xd, "fp32"), "f32out", f"patch_embed_mfma_{_xin(xd)}_f32out")


@pytest.mark.parametrize("case", E.F32OUT_REFUSALS, ids=[c[0] for c in E.F32OUT_REFUSALS])
def test_f32out_refusals(case):
    tag, R, S_, sh, sw, pad, flag = case
    N, C, H, W, K = 2, 3, 64, 72, 200
    x, w = _dev(np.zeros((N, C, H, W), np.float32), "fp32"), _dev(np.zeros((K, C, R, S_), np.float32))
    buf, y = _out_guarded((N, 64, K), "fp32")
    with _Flags((flag,) if flag else ()):
        assert _lib.load().mv_conv2d_nchw_f32out_supported(C, H, W, K, R, S_, sh, sw, pad, pad, F32) == 0, tag
        _refused(tag, "mv_conv2d_nchw_f32out_fwd", (_p(x), _p(w), None, None, _p(y), N, C, H, W, K, R, S_, sh, sw, pad, pad, 0, F32, 0, 0, None, _stream()), buf)


@pytest.mark.parametrize("mode", ["dyadic", "gauss"])
@pytest.mark.parametrize("xd", ["fp32", "bf16"])
@pytest.mark.parametrize("g", E.SPLIT_GEOMS, ids=E.geom_id)
def test_conv_split(g, xd, mode):
    """Two weight planes: w = a + b 2^-10 (every sum exact, ONE output rounding: equality with bf16_rne(ref)), and Gaussian hi + lo
    with K_red = 2 C R S.  C R S = 27 is padded to 32 in LDS: the pad columns of both planes must be zeros."""
    _run_nchw(E.nchw_case("split", mode, *g, xd, "bf16"), "split", f"stem_conv_mfma_{_xin(xd)}_w2")


@pytest.mark.parametrize("mode", ["int", "gauss"])
def test_generic_token_mode(mode):
    """force_generic on the patch16 geometry in token mode (tok_stride, tok_offset, pos): the same verdict as the fast kernel.  The
    fallback multiplies fp32 pixels as they are, so its images are bf16 values."""
    _run_nchw(E.nchw_case("plain", mode, *E.STEM_GEOMS[2], "fp32", "bf16", True), "fwd", "conv_generic", flags=("force_generic",))


# ================================================================================================ mv_linear_split_fwd
def _run_lsplit(tag, d, M, N, K, expect, flags=(), splitk=False):
    xd, wd = _dev(np.array(d["x"])), _dev(np.array(d["wcat"]))
    scd, shd, rd = _opt(d["scale"]), _opt(d["shift"]), _opt(d["res"], d["out"])
    buf, y = _out_guarded((M, N), d["out"])
    with _Flags(flags):
        assert _lib.load().mv_linear_split_supported(M, N, K, BF) == 1, tag
        if splitk:                                  # the mv_set_scratch protocol of include/eqxvision_amd.h
            nb = int(_lib.load().mv_splitk_scratch_bytes(M, N, 2 * K))
            assert nb > 0, f"{tag}: not a split shape"
            ws = torch.zeros(nb, dtype=torch.uint8, device="cuda")
            _lib.call("mv_set_scratch", _p(ws), nb, _stream())
        _lib.call("mv_linear_split_fwd", _p(xd), _p(wd), _p(scd), _p(shd), _p(rd), _p(y), M, N, K, d["act"], BF, DT[d["out"]], _stream())
        kern = _lib.last_kernel()
    torch.cuda.synchronize()
    if splitk:
        assert bool((ws[:4096] == 0).all().item()), f"{tag}: arrival words not left zero"
    assert _guard_ok(buf), f"{tag}: guard band behind y touched"
    _verdict(tag, kern, expect, "int" if d["info"] else "gauss", [("y", _host(y), d["ref"], d["mag"], d["kred"], d["out"])])


def _lsplit_kernel(tag, out):
    return f"igemm8_dual_bf16_{E.LSPLIT_TILES[tag]}" + ("_f32out" if out == "fp32" else "")


@pytest.mark.parametrize("epi", E.LSPLIT_EPILOGUES, ids=[e[0] for e in E.LSPLIT_EPILOGUES])
@pytest.mark.parametrize("shape", E.LSPLIT_SHAPES, ids=[s[0] for s in E.LSPLIT_SHAPES])
def test_linear_split_exact(shape, epi):
    """x integers, w = a + b 2^-10 split exactly into hi + lo, fp32 output: EQUAL to float64 at every tile, ragged edge and K."""
    tag, M, N, K = shape
    _run_lsplit(f"lsplit/{tag}/{epi[0]}/int", E.lsplit_case("int", M, N, K, *epi[1:], "fp32"), M, N, K, _lsplit_kernel(tag, "fp32"))


@pytest.mark.parametrize("out", ["fp32", "bf16"])
@pytest.mark.parametrize("shape", E.LSPLIT_SHAPES, ids=[s[0] for s in E.LSPLIT_SHAPES])
def test_linear_split_gauss(shape, out):
    """Gaussian fp32 weights split on the host; reference on hi + lo; the bound with K_red = 2 K."""
    tag, M, N, K = shape
    _run_lsplit(f"lsplit/{tag}/{out}/gauss", E.lsplit_case("gauss", M, N, K, True, True, True, 0, out), M, N, K, _lsplit_kernel(tag, out))


def test_linear_split_splitk_exact():
    """Scratch on offer and splitk_min_nk = 6: the launch splits its six k-tiles over two blocks; equality must survive."""
    tag, M, N, K = E.LSPLIT_SPLITK
    _run_lsplit(f"lsplit/{tag}/splitk/int", E.lsplit_case("int", M, N, K, True, True, True, 1, "fp32"), M, N, K,
                _lsplit_kernel(tag, "fp32") + "_splitk", flags=("splitk_min_nk=6",), splitk=True)


@pytest.mark.parametrize("case", E.LSPLIT_REFUSALS, ids=[c[0] for c in E.LSPLIT_REFUSALS])
def test_linear_split_refusals(case):
    tag, M, N, K, xdt, flag = case
    x, w = _dev(np.zeros((M, K), np.float32), xdt), _dev(np.zeros((N, 2 * K), np.float32))
    buf, y = _out_guarded((M, N), "fp32")
    with _Flags((flag,) if flag else ()):
        assert _lib.load().mv_linear_split_supported(M, N, K, DT[xdt]) == 0, tag
        _refused(tag, "mv_linear_split_fwd", (_p(x), _p(w), None, None, None, _p(y), M, N, K, 0, DT[xdt], F32, _stream()), buf)


# ================================================================================================ head-major stores
@pytest.mark.parametrize("mode", ["int", "gauss"])
@pytest.mark.parametrize("route", E.HEADS_ROUTES, ids=["+".join(r[0]) + ("" if r[1] else "noscale") or "rule" for r in E.HEADS_ROUTES])
@pytest.mark.parametrize("tokens", E.HEADS_TOKENS)
def test_linear_heads(tokens, route, mode):
    """The whole [B][3H][tokens][dh] buffer on both GEMM cores and each of their tiles; 197 and 50 tokens put image boundaries
    inside 256-row tiles.  The integer shift encodes the column: a swapped head or q / k / v group cannot cancel."""
    flags, with_scale, expect = route
    d = E.heads_case(mode, tokens, with_scale)
    M, N, K = d["M"], d["N"], d["K"]
    xd, wd, scd, shd = _dev(np.array(d["x"])), _dev(np.array(d["w"])), _opt(d["scale"]), _opt(d["shift"])
    buf, y = _out_guarded(d["ref"].shape)
    tag = f"heads/{tokens}/{'+'.join(flags) or 'rule'}/{mode}"
    with _Flags(flags):
        assert _lib.load().mv_linear_heads_supported(M, N, K, tokens, E.HEADS_DH, BF) == 1, tag
        _lib.call("mv_linear_heads_fwd", _p(xd), _p(wd), _p(scd), _p(shd), _p(y), M, N, K, tokens, E.HEADS_DH, BF, _stream())
        kern = _lib.last_kernel()
    torch.cuda.synchronize()
    assert _guard_ok(buf), f"{tag}: guard band behind y touched"
    _verdict(tag, kern, expect, mode, [("y", _host(y), d["ref"], d["mag"], d["kred"], "bf16")])


def test_lnin_head_major_is_a_permutation():
    """mv_linear_lnout_fwd -> mv_linear_lnin_fwd on 197 x 97 rows: the consumer's head-major result (tokens = 197, dh = 64) must be
    the exact permutation of its token-major result (tokens = 0) of the same planes and table, bit for bit; the token-major result
    within lnin_ref_bound and the bias rule as in tests/test_strict_lngemm_gpu.py::test_lnfold_pair."""
    case = G.LNFOLD_TOKEN_CASE
    M, D, Kp, N2, act, _ = case
    tokens = 197
    x, w, b, res, wf, cs, bfold = G.lnfold_data(*case)
    L = _lib.load()
    assert M % tokens == 0 and L.mv_linear_lnout_supported(M, D, Kp, BF) == 1
    assert L.mv_linear_lnin_supported(M, N2, D, 0, 0, BF) == 1 and L.mv_linear_lnin_supported(M, N2, D, tokens, 64, BF) == 1
    xd, wd, bd, rd = _dev(np.array(x)), _dev(np.array(w)), _dev(np.array(b), "fp32"), _dev(np.array(res), "fp32")
    P = -(-D // 256)
    (hbuf, hi), (lbuf, lo), (sbuf, st) = _out_guarded((M, D)), _out_guarded((M, D)), _out_guarded((P * M * 2,), "fp32")
    _lib.call("mv_linear_lnout_fwd", _p(xd), _p(wd), _p(bd), _p(rd), None, _p(hi), _p(lo), _p(st), M, D, Kp, BF, _stream())
    assert _lib.last_kernel() == "igemm8_bf16_256x256_lin_lnout_f32res"
    wfd, csd, bfd = _dev(np.array(wf)), _dev(np.array(cs), "fp32"), _dev(np.array(bfold), "fp32")
    out = {}
    for tk in (0, tokens):
        buf, y = _out_guarded((M, N2))
        _lib.call("mv_linear_lnin_fwd", _p(hi), _p(st), _p(wfd), _p(csd), _p(bfd), _p(y), M, N2, D, G.LNFOLD_EPS, act, tk, 64 if tk else 0, BF, _stream())
        assert _lib.last_kernel() == "igemm8_bf16_256x256_dense_lnin"
        torch.cuda.synchronize()
        assert _guard_ok(buf), f"lnin tokens={tk}: guard band behind y touched"
        out[tk] = y
    assert _guard_ok(hbuf) and _guard_ok(lbuf) and _guard_ok(sbuf)
    want = out[0].view(M // tokens, tokens, N2 // 64, 64).permute(0, 2, 1, 3).contiguous().view(torch.int16)
    diff = int((want != out[tokens].view(M // tokens, N2 // 64, tokens, 64).view(torch.int16)).sum().item())
    print(f"lnin head-major vs token-major: {diff} of {M * N2} elements differ in their bits")
    assert diff == 0
    ref, bound = G.lnin_ref_bound(_host(hi), _host(lo), wf, cs, bfold, act)
    got = _host(out[0])
    a, bi = N_.judge(got, ref, bound, "bf16")
    print(f"lnin tokens=0 [igemm8_bf16_256x256_dense_lnin]: worst |got-ref|/bound {a.get('worst', float('nan')):.3f}, violations {a.get('nviol')} | bias {bi['bias']:+.4f}")
    assert a["ok"] and bi["ok"], (a, bi)


# ================================================================================================ mv_vit_cls_pos_fwd
@pytest.mark.parametrize("D,out", E.CLS_POS_CASES)
def test_vit_cls_pos(D, out):
    """Row 0 of each image = cls + pos[0] (one fp32 add, one store); rows 1 .. 4 and the guard keep the sentinel."""
    cls, pos, ref, mag = E.cls_pos_case(D)
    clsd, posd = _dev(np.array(cls), "fp32"), _dev(np.array(pos), "fp32")
    buf, y = _out_guarded((E.CLS_B, E.CLS_T, D), out)
    _lib.call("mv_vit_cls_pos_fwd", _p(clsd), _p(posd), _p(y), E.CLS_B, E.CLS_T, D, DT[out], _stream())
    kern = _lib.last_kernel()
    torch.cuda.synchronize()
    got = _host(y)
    assert kern == "vit_cls_pos", kern
    assert _guard_ok(buf) and bool((got[:, 1:] == S.SENTINEL).all()), "cls_pos: a row other than row 0 was written"
    a = S.check_bound(got[:, 0], np.broadcast_to(ref, (E.CLS_B, D)), mag, 0, out, n_ops=1)
    print(f"cls_pos/D{D}/{out} [{kern}]: worst |got-ref|/bound {a.get('worst', float('nan')):.3f}, violations {a.get('nviol')}")
    assert a["ok"], a
    if out == "fp32":
        assert np.array_equal(got[:, 0], np.broadcast_to((cls + pos[0]).astype(np.float64), (E.CLS_B, D)))
