"""CPU proofs for the mixed-precision Swin window attention (tests/_swin_attn_mp_ref.py; the device side is
tests/test_swin_attn_mp_gpu.py).

1. The float64 formulas, with r = identity, agree with torch.autograd in float64 on the shifted-window attention core
   (tests/_strict.py: swin_bwd64: roll, partition, bias, mask, softmax, reverse), the bias gradient included.
2. Every construction holds (prove_exact_case) and the clean float32 emulation of the kernel passes every instrument at every shape
   of the GPU test.
3. Each of the ten seeded defects fails an instrument on at least one listed shape; where a defect cannot show on a shape, that is
   asserted with the reason.
4. The binding's signatures of the new entries exist.
"""
import ctypes

import numpy as np
import pytest

from tests import _strict as ST
from tests import _swin_attn_mp_ref as R

F64 = np.float64
IDS = [R.shape_id(s) for s in R.SHAPES]


def _ident(a):
    return np.asarray(a, F64)


# ================================================================================================ 1. the formulas
@pytest.mark.parametrize("shape", [R.SHAPES[1], R.SHAPES[2], R.SHAPES[3], R.SHAPES[6]], ids=[IDS[1], IDS[2], IDS[3], IDS[6]])
def test_formulas_match_autograd(shape):
    d = R.dims(shape)
    rng = np.random.default_rng(5)
    q, k, v, dout = (rng.standard_normal((d["G"], d["n"], d["dh"])) for _ in range(4))
    bias = 0.5 * rng.standard_normal((d["heads"], d["n"], d["n"]))
    c = {"shape": shape, "q": q, "k": k, "v": v, "dout": dout, "bias": bias, "scale": d["dh"] ** -0.5}
    f = R.fwd64(c, rnd=_ident)
    b = R.bwd64(c, f["out"], f["lse"], rnd=_ident)
    qkv = R.scatter(np.stack([q, k, v]), shape)
    dqkv, g = ST.swin_bwd64(qkv, bias, R.scatter(dout[None], shape), d["heads"], shape[5], shape[6])
    mine = R.scatter(np.stack([b["dq"], b["dk"], b["dv"]]), shape)
    np.testing.assert_allclose(mine, dqkv, rtol=1e-9, atol=1e-11)
    np.testing.assert_allclose(b["dbias"], g.sum(0), rtol=1e-9, atol=1e-11)
    np.testing.assert_allclose(b["g"].reshape(g.shape), g, rtol=1e-9, atol=1e-11)
    assert np.array_equal(R.gather(qkv, shape), np.stack([q, k, v]))                  # gather is the inverse of scatter


def test_parts_rule():
    assert R.parts_of((64, 56, 56, 96, 3, (7, 7), (3, 3))) == 682 and R.parts_of((4, 7, 7, 768, 24, (7, 7), (0, 0))) == 4
    assert all(R.parts_of(s) >= 1 for s in R.SHAPES)


# ================================================================================================ 2. the clean emulation
@pytest.mark.parametrize("shape", R.SHAPES, ids=IDS)
def test_clean_emulation_passes(shape):
    for kind in ("select", "tie", "flat"):
        if kind == "tie" and not R.has_tie(shape):
            continue
        p = R.exact_case(kind, shape)
        R.prove_exact_case(p)
        got = R.emulate(p)
        assert R.check_exact_fwd(got, p)["ok"], (kind, R.check_exact_fwd(got, p))
        if kind != "flat":
            assert R.check_exact_bwd(got, p)["ok"], (kind, R.check_exact_bwd(got, p))
    c = R.gauss_case(shape)
    info = R.check_gauss(R.emulate(c), c)
    print(f"swin_attn_mp/emulation/{R.shape_id(shape)}: worst error/bound {R.worst(info)}")
    assert info["ok"], info


def test_ties_exist_where_the_test_needs_them():
    """Every listed shape but the single key carries the tie."""
    assert [R.has_tie(s) for s in R.SHAPES] == [False, True, True, True, True, True, True]


# ================================================================================================ 3. the seeded defects
WORK, WORK0, N16, N6, N33, N64 = R.SHAPES[4], R.SHAPES[5], R.SHAPES[2], R.SHAPES[1], R.SHAPES[3], R.SHAPES[6]


def _exact(kind, shape, which, defect):
    p = R.exact_case(kind, shape)
    got = R.emulate(p, **{defect: True})
    return (R.check_exact_fwd if which == "fwd" else R.check_exact_bwd)(got, p)


def _gauss(shape, defect):
    c = R.gauss_case(shape)
    return R.check_gauss(R.emulate(c, **{defect: True}), c)


SEEN_BY = {
    "mask_ignored": lambda: _gauss(WORK, "mask_ignored")["out"],
    "mask_on_unshifted": lambda: _gauss(WORK0, "mask_on_unshifted")["out"],
    "pad_key_masked_by_minus100": lambda: _exact("flat", WORK, "fwd", "pad_key_masked_by_minus100")["out"],
    "bias_transposed": lambda: _exact("tie", N16, "fwd", "bias_transposed")["out"],
    "bias_wrong_head": lambda: _exact("select", N16, "fwd", "bias_wrong_head")["lse"],
    "roll_wrong_sign": lambda: _gauss(N6, "roll_wrong_sign")["out"],
    "q_prescaled_before_round": lambda: _gauss(WORK, "q_prescaled_before_round")["lse"],
    "dbias_from_rounded_g": lambda: _gauss(WORK, "dbias_from_rounded_g")["dbias"],
    "dbias_drops_last_window": lambda: _gauss(N33, "dbias_drops_last_window")["dbias"],
    "dbias_part_overwritten": lambda: _gauss(R.WALK_SHAPES[0], "dbias_part_overwritten")["dbias"],
}


def test_every_defect_has_an_instrument():
    assert set(SEEN_BY) == set(R.DEFECTS) and len(R.DEFECTS) >= 9


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_defect_is_seen(defect):
    info = SEEN_BY[defect]()
    assert not info["ok"], f"{defect} passed its instrument: {info}"


def test_gauss_sees_the_bias_defects_too():
    assert not _gauss(WORK, "bias_transposed")["out"]["ok"]
    assert not _gauss(WORK, "bias_wrong_head")["out"]["ok"]
    assert not _gauss(WORK, "roll_wrong_sign")["dq"]["ok"]


def test_where_a_defect_cannot_show():
    """mask_on_unshifted on a shifted map: the mask is already there.  mask_ignored on an unshifted map: there is no mask.
    pad_key_masked_by_minus100 at n = 64: there is no padding.  bias_wrong_head with one head: (h + 1) % 1 = h.
    q_prescaled_before_round at dh = 64: the scale 1 / 8 is a power of two, so r(q / 8) = r(q) / 8 and nothing changes."""
    for shape, defect in ((WORK, "mask_on_unshifted"), (WORK0, "mask_ignored"), (N64, "pad_key_masked_by_minus100"),
                          (N33, "bias_wrong_head"), (N64, "q_prescaled_before_round")):
        c = R.gauss_case(shape)
        a, b = R.emulate(c), R.emulate(c, **{defect: True})
        assert all(np.array_equal(a[t], b[t]) for t in R.OUTS), (R.shape_id(shape), defect)


# ------------------------------------------------------------------------------------------------ more than one window per workgroup
WALK_IDS = [R.shape_id(s) for s in R.WALK_SHAPES]


def test_walk_shapes_walk():
    """Both walk shapes have W = 2 with a ragged last round; every shape of SHAPES (raised to its Gaussian batch) has W = 1."""
    for s in R.WALK_SHAPES:
        d = R.dims(R.gauss_shape(s))
        assert R.gauss_shape(s) == s and R.walk_len(s) == 2 and (d["B"] * d["nW"]) % R.parts_of(s) != 0
    assert [R.parts_of(s) for s in R.WALK_SHAPES] == [2048, 682]
    assert all(R.walk_len(R.gauss_shape(s)) == 1 for s in R.SHAPES)


@pytest.mark.parametrize("shape", R.WALK_SHAPES, ids=WALK_IDS)
def test_clean_emulation_passes_where_a_workgroup_walks_two_windows(shape):
    """(The 2064 groups of the 7 x 7 shape take the tie and the Gaussian case only: each construction costs seconds there.)"""
    for kind in ("select", "tie", "flat") if shape == R.WALK_SHAPES[0] else ("tie",):
        assert R.has_tie(shape)
        p = R.exact_case(kind, shape)
        R.prove_exact_case(p)
        got = R.emulate(p)
        assert R.check_exact_fwd(got, p)["ok"], (kind, R.check_exact_fwd(got, p))
        if kind != "flat":
            assert R.check_exact_bwd(got, p)["ok"], (kind, R.check_exact_bwd(got, p))
    c = R.gauss_case(shape)
    info = R.check_gauss(R.emulate(c), c)
    print(f"swin_attn_mp/emulation/{R.shape_id(shape)}: worst error/bound {R.worst(info)}")
    assert info["ok"], info


def test_dbias_defects_are_seen_where_a_workgroup_walks_two_windows():
    """The W term of the dbias bound and the three dbias instruments at W = 2, on the 7 x 7 shape (688 windows on 682 parts).  The
    dropped pair is the last one, which its part adds SECOND: that part is not empty, it is short of one window.  A part that keeps
    only the last window it walked shows at the 2 x 2 shape as well; the other two do not there, and are not asked to: its dbias has
    16 elements, each the sum of 2080 windows, and the bound -- the sum of the windows' own worst cases -- exceeds one window's g."""
    big, small = R.WALK_SHAPES[1], R.WALK_SHAPES[0]
    c = R.gauss_case(big)
    for defect in ("dbias_drops_last_window", "dbias_from_rounded_g", "dbias_part_overwritten"):
        info = R.check_gauss(R.emulate(c, **{defect: True}), c)["dbias"]
        assert not info["ok"], f"{defect} passed at W = 2: {info}"
    assert not _gauss(small, "dbias_part_overwritten")["dbias"]["ok"]


def test_overwritten_part_cannot_show_at_one_window():
    c = R.gauss_case(WORK)
    a, b = R.emulate(c), R.emulate(c, dbias_part_overwritten=True)
    assert all(np.array_equal(a[t], b[t]) for t in R.OUTS)


# ================================================================================================ 4. the binding
def test_lib_signatures():
    from eqxvision_amd import _lib
    P = _lib.PROTOTYPES
    assert len(P["mv_swin_attn_mp_supported"]) == 2 and len(P["mv_swin_attn_mp_bwd_parts"]) == 6
    fwd, bwd = P["mv_swin_attn_mp_fwd"], P["mv_swin_attn_mp_bwd"]
    assert len(fwd) == 15 and fwd[:4] == [ctypes.c_void_p] * 4 and fwd[13] is ctypes.c_float and fwd[14] is ctypes.c_void_p
    assert len(bwd) == 18 and bwd[:7] == [ctypes.c_void_p] * 7 and bwd[16] is ctypes.c_float and bwd[17] is ctypes.c_void_p
    assert all(t is ctypes.c_int for t in fwd[4:13] + bwd[7:16])
