"""CPU: the instruments of tests/_strict_attn.py on every construction and shape of tests/test_strict_attn_gpu.py -- the host proofs
hold, the clean emulation of the MFMA arithmetic passes every instrument, and each defect is rejected by the instrument named for
it.  For every defect the line `old criterion: passes / fails` records whether tests/_cases.py::_cmp would have seen it (`-s`)."""
import numpy as np
import pytest

from tests import _strict as ST
from tests import _strict_attn as A
from tests import _swin_v2_ref as R

MFMA_MHA = A.MHA_SHAPES + A.MHA_HM_SHAPES[1:]
ALL_MHA = MFMA_MHA + tuple(s[:4] for s in A.MHA_OTHER)
ALL_SWIN = A.SWIN_SHAPES + (A.SWIN_OTHER[1][:6],) + tuple(s for s in A.COS_SHAPES if s not in A.SWIN_SHAPES)
_ids = lambda shapes: ["x".join(str(v) for v in s) for s in shapes]


def _old(tag, defect, got, ref, tol=1e-2):
    print(f"{tag} {defect}: old criterion {'passes' if A.old_cmp(got, ref, tol) else 'fails'}")


# ------------------------------------------------------------------------------------------------ proofs + clean emulation
@pytest.mark.parametrize("shape", ALL_MHA, ids=_ids(ALL_MHA))
def test_mha_constructions_clean(shape):
    mfma = shape[3] in (32, 64)
    for kind in ("select", "tie", "flat"):
        p = A.mha_problem(kind, shape, 3)
        gap = A.prove(p)
        if not mfma:
            continue
        out, pr = A.emulate(p)
        i1, i2 = A.check_exactish(kind, out, p), A.check_probs(kind, pr, p)
        print(f"mha {shape} {kind}: gap {gap:.0f} out {i1['worst']} probs {i2['worst']:.3f}")
        assert i1["ok"] and i2["ok"], (kind, i1, i2)
    if mfma:
        p = A.mha_problem("gauss", A.gauss_shape(shape), 4)
        out, pr = A.emulate(p)
        i1, i2 = A.check_gauss(out, p), A.check_gauss_probs(pr, p)
        print(f"mha {shape} gauss: worst {i1['worst']:.3f} bias {i1['bias']:+.4f} over {i1['n_bias']} probs {i2['worst']:.3f}")
        assert i1["ok"] and i2["ok"], (i1, i2)


@pytest.mark.parametrize("shape", ALL_SWIN, ids=_ids(ALL_SWIN))
def test_swin_constructions_clean(shape):
    B, Hf, C, heads, ws, shift = shape
    mfma = C // heads == 32
    cases = [("select", True), ("select", False), ("tie", True), ("tie", False), ("flat", True)]
    if A.eff_shift(Hf, ws, shift):
        cases.append(("mask", True))
    for kind, by_bias in cases:
        p, extra = A.swin_problem(kind, shape, 5, by_bias)
        gap = A.prove(p, extra)
        if not mfma:
            continue
        out, _ = A.emulate(p, extra, n_pad=64)
        info = A.check_exactish(kind, out, p)
        print(f"swin {shape} {kind} {'bias' if by_bias else 'codes'}: gap {gap:.0f} out {info['worst']}")
        assert info["ok"], (kind, by_bias, info)
    if mfma:
        p, extra = A.swin_problem("gauss", shape, 6)
        out, _ = A.emulate(p, extra, n_pad=64)
        info = A.check_gauss(out, p, extra)
        print(f"swin {shape} gauss: worst {info['worst']:.3f} bias {info['bias']:+.4f} over {info['n_bias']}")
        assert info["ok"], info
    mk = R.shift_mask(Hf, Hf, [ws, ws], [shift, shift])                 # the restatement's mask anchors region_map
    reg = A.region_map(Hf, ws, shift)
    mine = np.where(reg[:, :, None] != reg[:, None, :], -100.0, 0.0)
    assert (not mine.any()) if mk is None else np.array_equal(mine, mk.numpy())
    if A.eff_shift(Hf, ws, shift):
        sizes = sorted({int(c) for r in A.region_map(Hf, ws, shift) for c in np.bincount(r) if c})
        print(f"swin {shape}: region sizes {sizes}")
        if (ws, shift) == (7, 3):
            assert sizes == [9, 12, 16, 21, 28, 49]


# ------------------------------------------------------------------------------------------------ defects
@pytest.mark.parametrize("shape", MFMA_MHA, ids=_ids(MFMA_MHA))
def test_mha_defects_rejected(shape):
    B, N, H, dh = shape
    tag = f"mha {shape}"
    sel, tie, flat = (A.mha_problem(k, shape, 3) for k in ("select", "tie", "flat"))
    gs = A.mha_problem("gauss", A.gauss_shape(shape), 4)
    gref, _, _, gpr = A.ref64(gs)
    for d in ("drop_last_key", "swap_keys_in_step"):
        out, _ = A.emulate(sel, **{d: True})
        assert not A.check_exactish("select", out, sel)["ok"], d
        _old(tag, d, A.emulate(gs, **{d: True})[0], gref)
    if N % 32:
        out, _ = A.emulate(flat, unmasked_pad=True)
        assert not A.check_exactish("flat", out, flat)["ok"]
        _old(tag, "unmasked_pad", A.emulate(gs, unmasked_pad=True)[0], gref)
    if N > 4:
        out, pr = A.emulate(tie, no_half_exchange=True)
        assert not A.check_exactish("tie", out, tie)["ok"] and not A.check_probs("tie", pr, tie)["ok"]
        _old(tag, "no_half_exchange", A.emulate(gs, no_half_exchange=True)[0], gref)
    out, pr = A.emulate(gs, scale_off=True)
    assert not A.check_gauss(out, gs)["ok"] and not A.check_gauss_probs(pr, gs)["ok"]
    _old(tag, "scale_off", out, gref)
    _old(tag, "scale_off (probs)", pr, gpr, 2e-3)
    out, _ = A.emulate(gs, truncate_p=True)
    info = A.check_gauss(out, gs)
    print(f"{tag} truncate_p: worst {info['worst']:.3f} bias {info['bias']:+.4f} over {info['n_bias']}")
    assert info["n_bias"] >= ST.BIAS_MIN_ELEMS and abs(info["bias"]) > ST.BIAS_LIMIT and not info["ok"], info
    _old(tag, "truncate_p", out, gref)
    for p, kind in ((sel, "select"), (tie, "tie"), (flat, "flat")):
        _, pr = A.emulate(p, probs_unnormalised=True)
        if kind != "select":                                   # one exponential: the sum IS that exponential
            assert not A.check_probs(kind, pr, p)["ok"], kind
    km = 2.0 * (ST.rng_of(8).random((B * H, N, N)) < 0.5)              # attention dropout at p = 0.5: 1 / keep = 2 is exact
    assert ((sel["win"] * km).sum(-1) == 0).any() and ((sel["win"] * km).sum(-1) == 2).any()
    for p, kind in ((sel, "select"), (tie, "tie")):
        out, pr = A.emulate(p, keepmask=km)
        i1, i2 = ST.check_exact(out, A.expect_dropped(p, km)), A.check_probs(kind, pr, p, km)
        assert i1["ok"] and i2["ok"], (kind, i1, i2)
        out, pr = A.emulate(p, keepmask=km, drop_last_key=True)
        assert not ST.check_exact(out, A.expect_dropped(p, km))["ok"]
    _, pr = A.emulate(gs, probs_unnormalised=True)
    assert not A.check_gauss_probs(pr, gs)["ok"]
    _old(tag, "probs_unnormalised (probs)", pr, gpr, 2e-3)


MFMA_SWIN = tuple(s for s in ALL_SWIN if s[2] // s[3] == 32)


@pytest.mark.parametrize("shape", MFMA_SWIN, ids=_ids(MFMA_SWIN))
def test_swin_defects_rejected(shape):
    B, Hf, C, heads, ws, shift = shape
    n = ws * ws
    tag = f"swin {shape}"
    gs, gx = A.swin_problem("gauss", shape, 6)
    gref = A.ref64(gs, gx)[0]
    for by_bias in (True, False):
        sel, sx = A.swin_problem("select", shape, 5, by_bias)
        for d in ("drop_last_key", "swap_keys_in_step"):
            out, _ = A.emulate(sel, sx, n_pad=64, **{d: True})
            assert not A.check_exactish("select", out, sel)["ok"], (d, by_bias)
        tie, tx = A.swin_problem("tie", shape, 5, by_bias)
        out, _ = A.emulate(tie, tx, n_pad=64, no_half_exchange=True)
        assert not A.check_exactish("tie", out, tie)["ok"], by_bias
    for d in ("drop_last_key", "swap_keys_in_step", "no_half_exchange"):
        _old(tag, d, A.emulate(gs, gx, n_pad=64, **{d: True})[0], gref)
    if n < 64:
        flat, fx = A.swin_problem("flat", shape, 5)
        out, _ = A.emulate(flat, fx, n_pad=64, unmasked_pad=True)
        assert not A.check_exactish("flat", out, flat)["ok"]
        _old(tag, "unmasked_pad", A.emulate(gs, gx, n_pad=64, unmasked_pad=True)[0], gref)
    out, _ = A.emulate(gs, gx, n_pad=64, scale_off=True)
    assert not A.check_gauss(out, gs, gx)["ok"]
    _old(tag, "scale_off", out, gref)
    out, _ = A.emulate(gs, gx, n_pad=64, truncate_p=True)
    info = A.check_gauss(out, gs, gx)
    print(f"{tag} truncate_p: worst {info['worst']:.3f} bias {info['bias']:+.4f} over {info['n_bias']}")
    assert info["n_bias"] >= ST.BIAS_MIN_ELEMS and abs(info["bias"]) > ST.BIAS_LIMIT and not info["ok"], info
    _old(tag, "truncate_p", out, gref)
    if A.eff_shift(Hf, ws, shift):
        mk, mx = A.swin_problem("mask", shape, 5)
        _, bad = A.swin_problem("mask", shape, 5, off_by_one=True)
        out, _ = A.emulate(mk, bad, n_pad=64)
        assert not A.check_exactish("mask", out, mk)["ok"]
        _, gbad = A.swin_problem("gauss", shape, 6, off_by_one=True)
        _old(tag, "mask_region_off_by_one", A.emulate(gs, gbad, n_pad=64)[0], gref)
