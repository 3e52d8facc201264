"""CPU proofs for tests/test_strict_entry_gpu.py (instruments, constructions and emulations: tests/_strict_entry.py).

Every construction's preconditions are asserted when the case is built (prove_visible, prove_dyadic, S.prove_exact); the honest
float32 emulation of each contract passes both instruments on the data the GPU module uses; each seeded defect is rejected by at
least one of them.  Where a defect is NOT rejected, and why:

    truncate_x / half_up_x    on every bf16-valued image (modes "int", "dyadic", bf16 images): nothing to round -- that is the gap
                              the rounding-visible cases close; asserted below (test_bf16_valued_images_cannot_see_operand_rounding)
    half_up_x                 on the un-rounded Gaussian images: a Gaussian fp32 value is never an exact tie; left to the visible cases
    truncate_x                on the un-rounded Gaussian images it is NOT reliably outside elem_bound (the operand error of half a bf16
                              ulp per pixel averages out over the reduction); the visible cases reject it on every entry
    truncate_store            invisible to the exact cases whose outputs are bf16 values (nothing to round) and to fp32 outputs;
                              rejected by the bias rule and by the dyadic split conv (one rounding of an exact value)
    image_index_per_tile      at tokens = 256 (tiles never straddle an image: the aligned control)
    lo_pad_garbage            where C R S is a multiple of 16 (no pad columns); remainder_rows_read where H % R == 0
"""
import numpy as np
import pytest

from tests import _strict as S
from tests import _strict_entry as E

SEEN = set()                   # (defect, instrument) pairs that rejected, filled by the tests and read by the last one


def _judge(ref, mag, kred, out, exact, got):
    """ok under the case's instrument(s): equality, or every element inside elem_bound and the bias rule where it applies."""
    if exact:
        return S.check_exact(got, ref)["ok"], "exact"
    a = S.check_bound(got, ref, mag, kred, out)
    eligible = int((np.abs(ref) >= 2.0 ** -6).sum())
    if out == "bf16" and kred <= S.BIAS_MAX_KRED and eligible >= S.BIAS_MIN_ELEMS and a["ok"]:
        return S.check_bias(got, ref, out)["ok"], "bias"
    return a["ok"], "bound"


def _reject(name, ok, how, defect):
    assert not ok, f"{name}: defect {defect} passes"
    SEEN.add(defect)
    print(f"   {name}: {defect} rejected by {how}")


# ================================================================================================ A. rounding-visible operands
VISIBLE = [("plain", g, "bf16") for g in E.STEM_GEOMS] + [("plain", E.F32OUT_GEOMS[0], "fp32")] + [("split", g, "bf16") for g in E.SPLIT_GEOMS]


@pytest.mark.parametrize("kind,g,out", VISIBLE, ids=[f"{k}/{g[0]}/{o}" for k, g, o in VISIBLE])
def test_visible_case(kind, g, out):
    """prove_visible holds (asserted in nchw_case: >= 25 % ties, >= 25 % truncation-visible, every output a bf16 value), the honest
    emulation EQUALS the reference, and the two operand-rounding defects change more than 10 % of the outputs."""
    d = E.nchw_case(kind, "visible", *g, "fp32", out)
    f = d["info"]
    print(f"{kind}/{g[0]}: ties {f['ties']:.3f} trunc differs {f['trunc_differs']:.3f} half-up differs {f['half_up_differs']:.3f}")
    assert f["ties"] >= 0.25 and f["trunc_differs"] >= 0.25
    assert S.check_exact(E.emu_nchw(d), d["full"])["ok"]
    for defect in ("truncate_x", "half_up_x"):
        e = S.check_exact(E.emu_nchw(d, defect), d["full"])
        changed = e["nbad"] / d["ref"].size
        print(f"   {defect}: {100 * changed:.1f} % of the outputs change")
        assert changed > 0.10, (defect, changed)
        _reject(g[0], e["ok"], "exact", defect)
    if kind == "split":
        for defect in ("drop_lo", "lo_k_shift") + (("lo_pad_garbage",) if (3 * g[5] * g[5]) % 16 else ()):
            _reject(g[0], S.check_exact(E.emu_nchw(d, defect), d["full"])["ok"], "exact", defect)


@pytest.mark.parametrize("g", E.POOL_GEOMS, ids=E.geom_id)
def test_visible_stem_pool(g):
    tag, N, H, W, R, stride, pad, pp, with_scale, _ = g
    p = E.pool_case(tag, N, H, W, R, stride, pad, pp, with_scale)
    f = p["info"]
    assert f["ties"] >= 0.25 and f["trunc_differs"] >= 0.25
    assert S.check_exact(E.emu_nchw(None, pooled=p), p["ref"])["ok"]
    for defect in ("truncate_x", "half_up_x"):
        e = S.check_exact(E.emu_nchw(None, defect, pooled=p), p["ref"])
        assert e["nbad"] / p["ref"].size > 0.10, (defect, e["nbad"])
        _reject(tag, e["ok"], "exact", defect)


def test_bf16_valued_images_cannot_see_operand_rounding():
    """The gap: on the operands of the earlier strict cases (integers, bf16-valued Gaussians) a truncating or half-up operand
    conversion is bit-identical to the honest one."""
    for mode in ("int", "gauss"):
        d = E.nchw_case("plain", mode, *E.STEM_GEOMS[0], "fp32", "bf16", True)
        for defect in ("truncate_x", "half_up_x"):
            assert np.array_equal(E.emu_nchw(d, defect), E.emu_nchw(d))


# ================================================================================================ B. NCHW entry variants
def _nchw_verdict(d, got):
    body = got[:, 1:] if d["T"] else got
    ok, how = _judge(d["ref"], d["mag"], d["kred"], d["out"], d["exact"], body)
    if d["T"] and not bool((got[:, 0] == S.SENTINEL).all()):
        return False, "sentinel"
    return ok, how


B_CASES = ([("plain", m, g, xd, "bf16") for g in E.STEM_GEOMS for xd in ("bf16",) for m in ("int", "gauss")]
           + [("plain", m, g, xd, "fp32") for g in E.F32OUT_GEOMS for xd in ("fp32", "bf16") for m in ("int", "gauss")]
           + [("split", m, g, xd, "bf16") for g in E.SPLIT_GEOMS for xd in ("fp32", "bf16") for m in ("dyadic", "gauss")])


@pytest.mark.parametrize("kind,mode,g,xd,out", B_CASES, ids=[f"{k}/{g[0]}/{xd}/{o}/{m}" for k, m, g, xd, o in B_CASES])
def test_nchw_variants(kind, mode, g, xd, out):
    d = E.nchw_case(kind, mode, *g, xd, out)
    ok, how = _nchw_verdict(d, E.emu_nchw(d))
    assert ok, (how, g[0])
    defects = []
    if d["T"]:
        defects += ["pos_off_by_one", "cls_row_written"]
    if d["stride"] == d["R"] and d["H"] % d["R"]:
        defects += ["remainder_rows_read"]
    if kind == "split":
        defects += ["drop_lo", "lo_k_shift"] + (["lo_pad_garbage"] if (3 * d["R"] ** 2) % 16 else [])
        if mode == "dyadic":
            defects += ["truncate_store"]
            print(f"   lo plane non-zero: {100 * d['info']['lo_nonzero']:.0f} %")
    if out == "bf16" and mode == "gauss" and d["ref"].size >= 4 * S.BIAS_MIN_ELEMS and d["kred"] <= S.BIAS_MAX_KRED:
        defects += ["truncate_store"]
    for defect in defects:
        ok, how = _nchw_verdict(d, E.emu_nchw(d, defect))
        _reject(f"{kind}/{g[0]}/{mode}", ok, how, defect)


# ================================================================================================ C. mv_linear_split_fwd
def test_lsplit_shapes_reach_every_tile():
    """The table's tiles are what route_linear_split's rule gives, all three occur, both K occur at both half-size tiles, and the
    split-K case engages with splitk_min_nk = 6 (and not with the default 40)."""
    for tag, M, N, K in E.LSPLIT_SHAPES:
        assert E.split_tile(M, N, K)[0] == E.LSPLIT_TILES[tag], tag
        assert K % 64 == 0 and N % 8 == 0
    assert set(E.LSPLIT_TILES.values()) == {"256x256", "128x256", "256x128"}
    for tile in ("128x256", "256x128"):
        assert {K for tag, M, N, K in E.LSPLIT_SHAPES if E.LSPLIT_TILES[tag] == tile} == {64, 192}
    assert E.split_tile(74 * 256, 264, 192)[0] != "256x256" and E.split_tile(74 * 256 + 1, 256, 192)[0] != "256x256"
    _, M, N, K = E.LSPLIT_SPLITK
    assert E.split_tile(M, N, K, 6)[1] and not E.split_tile(M, N, K)[1]


LS_SMALL = [s for s in E.LSPLIT_SHAPES if s[1] <= 300]


@pytest.mark.parametrize("epi", E.LSPLIT_EPILOGUES, ids=[e[0] for e in E.LSPLIT_EPILOGUES])
@pytest.mark.parametrize("shape", LS_SMALL, ids=[s[0] for s in LS_SMALL])
def test_lsplit_exact(shape, epi):
    _, M, N, K = shape
    d = E.lsplit_case("int", M, N, K, *epi[1:], "fp32")
    assert d["info"]["lo_nonzero"] >= 0.5
    assert S.check_exact(E.emu_lsplit(d), d["ref"])["ok"]
    for defect in ("drop_lo", "lo_k_shift"):
        e = S.check_exact(E.emu_lsplit(d, defect), d["ref"])
        if defect == "drop_lo" and M * N >= 1024 and epi[4] == 0:
            assert e["nbad"] / d["ref"].size > 0.9
        _reject(shape[0], e["ok"], "exact", defect)


@pytest.mark.parametrize("out", ["fp32", "bf16"])
@pytest.mark.parametrize("shape", LS_SMALL, ids=[s[0] for s in LS_SMALL])
def test_lsplit_gauss(shape, out):
    _, M, N, K = shape
    d = E.lsplit_case("gauss", M, N, K, True, True, True, 0, out)
    ok, how = _judge(d["ref"], d["mag"], d["kred"], out, False, E.emu_lsplit(d))
    assert ok, how
    for defect in ("drop_lo", "lo_k_shift") + (("truncate_store",) if out == "bf16" and M * N >= 4 * S.BIAS_MIN_ELEMS else ()):
        if defect == "drop_lo" and out == "bf16":
            continue                                  # the lo term is below half a bf16 ulp of most outputs: the fp32 form shows it
        ok, how = _judge(d["ref"], d["mag"], d["kred"], out, False, E.emu_lsplit(d, defect))
        _reject(f"{shape[0]}/{out}", ok, how, defect)


# ================================================================================================ D. head-major stores
def _heads_verdict(d, mode, buf):
    n = d["M"] * d["N"]
    if not bool((buf[n:] == S.SENTINEL).all()):
        return False, "guard"
    return _judge(d["ref"], d["mag"], d["kred"], "bf16", mode == "int", buf[:n].reshape(d["ref"].shape))


@pytest.mark.parametrize("mode", ["int", "gauss"])
@pytest.mark.parametrize("tokens", E.HEADS_TOKENS)
def test_heads(tokens, mode):
    d = E.heads_case(mode, tokens, True)
    assert d["M"] >= 4096 and d["M"] - tokens < 4096 and ((d["M"] // tokens > 1 and tokens % 256 != 0) == (tokens != 256))
    ok, how = _heads_verdict(d, mode, E.emu_heads(d))
    assert ok, how
    for defect in E.HEADS_DEFECTS:
        if defect == "truncate_store" and mode == "int":
            continue
        ok, how = _heads_verdict(d, mode, E.emu_heads(d, defect))
        if defect == "image_index_per_tile" and tokens == 256:
            assert ok                                  # the aligned control: nothing changes
            continue
        _reject(f"heads/{tokens}/{mode}", ok, how, defect)


def test_heads_routes_cover_both_cores():
    assert len({k for _, _, k in E.HEADS_ROUTES}) == 7
    assert {k.split("_")[0] for _, _, k in E.HEADS_ROUTES} == {"igemm8", "igemm2"}


# ================================================================================================ mv_vit_cls_pos_fwd
@pytest.mark.parametrize("D,out", E.CLS_POS_CASES)
def test_cls_pos(D, out):
    cls, pos, ref, mag = E.cls_pos_case(D)

    def verdict(y):
        rest = np.delete(y, 0, axis=1)
        return S.check_bound(y[:, 0], np.broadcast_to(ref, (E.CLS_B, D)), mag, 0, out, n_ops=1)["ok"] and bool((rest == S.SENTINEL).all())
    assert verdict(E.emu_cls_pos(cls, pos, out))
    for defect in ("pos_off_by_one", "stride_ignored"):
        assert not verdict(E.emu_cls_pos(cls, pos, out, defect)), defect
    if out == "bf16":                                   # a truncated sum is off by up to a whole ulp: outside n_ops = 1 somewhere in D
        assert not verdict(E.emu_cls_pos(cls, pos, out, "truncate_store"))


def test_zz_every_listed_defect_was_rejected_somewhere():
    """The issue's twelve switches: each was rejected by an instrument in a test above (this test runs last in the module)."""
    listed = {"truncate_x", "half_up_x", "drop_lo", "lo_k_shift", "lo_pad_garbage", "remainder_rows_read", "pos_off_by_one",
              "cls_row_written", "token_major_store", "image_index_per_tile", "qkv_group_swap", "truncate_store"}
    if SEEN:                                            # (selected alone, nothing has been recorded)
        assert listed <= SEEN, listed - SEEN
