"""CPU proofs for tests/test_strict_swinblock_gpu.py: the float32 emulation of mv_swin_block_attn_fwd's four kernels
(tests/_strict_swinblock.py: emulate) goes through the instruments the GPU module uses, at the rectangular map 14 x 21 with shifts
(2, 5).  The honest emulation passes every instrument at every kernel; each seeded defect, one switch at a time, is rejected by at
least one -- or is listed in W.NOT_REJECTED with the reason, and printed as such.  The table (-s) names the instruments that reject
each defect and whether the former `_cmp(got, ref, 1e-2)` lets it through on the same Gaussian data; the module docstring of
tests/_strict_swinblock.py records it.
"""
import functools

import numpy as np
import pytest

from tests import _strict_attn as A
from tests import _strict_swinblock as W

KERNELS = list(W.KERNELS)


@functools.lru_cache(maxsize=None)
def _verdicts(kernel, defect):
    """({instrument: info}, passes _cmp at 1e-2 on the Gaussian data)."""
    out, cmp_ok = {}, None
    for name, op in W.instruments(kernel, W.HOST_GEOM):
        got = W.emulate(kernel, op, defect)
        out[name] = W.check(op, got)
        if name == "gauss":
            cmp_ok = A.old_cmp(got, op["ref"], 1e-2)
    return out, cmp_ok


def _applies(kernel, defect):
    C, nwin = W.KERNELS[kernel][:2]
    if defect == "window_pair_swap":
        return nwin == 2
    return True


# ================================================================================================ geometry and constructions
def test_geometry_restatements():
    # the gather is a permutation of the rows, the identity partition without a shift, and the roll moves (shh, shw) to window 0 token 0
    for B, Hf, Wf, shh, shw in W.GEOMS + W.GEOMS_ODD:
        idx = W.tok_index(B, Hf, Wf, shh, shw)
        assert sorted(idx.reshape(-1).tolist()) == list(range(B * Hf * Wf))
        assert idx[0, 0, 0] == shh * Wf + shw and idx[0, 0, 1] == shh * Wf + shw + 1 and idx[0, 0, 7] == (shh + 1) * Wf + shw
        reg = W.region_map(Hf, Wf, shh, shw)
        assert reg.shape == ((Hf // 7) * (Wf // 7), 49)
        if shh + shw == 0:
            assert not reg.any()
        else:
            # the last window sees all of its axis classes; the first window is one region; classes are constant per region and window
            assert len(np.unique(reg[-1])) == 4 and len(np.unique(reg[0])) == 1
            cls = W.mask_classes(shh, shw)
            for w in range(reg.shape[0]):
                for c in np.unique(cls):
                    assert len(np.unique(reg[w][cls == c])) == 1
            # the kernel's arithmetic, restated independently: rh = (yy < Hf - 7) ? 0 : (yy < Hf - shh ? 1 : 2), the same in x
            yy, xx = np.arange(Hf)[:, None], np.arange(Wf)[None, :]
            rh = np.where(yy < Hf - 7, 0, np.where(yy < Hf - shh, 1, 2))
            rw = np.where(xx < Wf - 7, 0, np.where(xx < Wf - shw, 1, 2))
            m = (3 * rh + rw).reshape(Hf // 7, 7, Wf // 7, 7).transpose(0, 2, 1, 3).reshape(-1, 49)
            assert np.array_equal(m, reg)
    # 21 x 21, shifted: the interior window (4 of 9) has region 0 throughout
    assert not W.region_map(21, 21, 3, 3)[4].any() and W.region_map(21, 21, 3, 3)[8].any()
    assert not np.array_equal(W.region_map(14, 21, 2, 5), W.region_map(14, 21, 5, 2))
    assert not np.array_equal(W.region_map(14, 21, 3, 3), W.region_map(14, 21, 3, 3, off_by_one=True))


def test_case_table():
    ids = [W.case_id(c) for c in W.CASES]
    assert len(set(ids)) == len(ids)
    for k, (C, nwin, _, _) in W.KERNELS.items():
        geoms = [g for kk, g in W.CASES if kk == k]
        assert {(g[1], g[2]) for g in geoms} >= {(14, 14), (14, 21), (21, 14)}
        assert {(g[3], g[4]) for g in geoms} == {(0, 0), (3, 3), (2, 5)}
        assert (((21, 21) in {(g[1], g[2]) for g in geoms}) == (nwin == 1))
        for g in geoms:
            assert ((g[1] // 7) * (g[2] // 7)) % nwin == 0


@pytest.mark.parametrize("kernel", KERNELS)
def test_constructions_are_proved(kernel):
    """Building an instrument runs its proofs (prove_pm1, A.prove, S.prove_exact, distinct v); the honest fragment IS +-1."""
    C, _, _, lnkind = W.KERNELS[kernel]
    for name, op in W.instruments(kernel, W.HOST_GEOM):
        if name != "gauss":
            x = np.asarray(op["x"]).reshape(-1, C)
            n = W.G._normalise(x, W.EPS, lnkind, None)
            assert set(np.unique(n).tolist()) == {-1.0, 1.0}, (kernel, name)
    # a construction that breaks a precondition is refused: winners that are not alone at the top
    op = W.exact_b(kernel, W.HOST_GEOM)
    B, Hf, Wf, shh, shw = W.HOST_GEOM
    idx, reg = W.tok_index(B, Hf, Wf, shh, shw), W.region_map(Hf, Wf, shh, shw)
    sg = np.sign(op["x"].reshape(-1, C) - op["x"].reshape(-1, C).mean(1, keepdims=True)).astype(np.float64)
    t = sg @ op["wqkv"].astype(np.float64).T
    q, k = (W.to_groups(t[:, i * C:(i + 1) * C], idx, C // 32) for i in range(2))
    win = np.zeros((q.shape[0], 49, 49), bool)
    win[:, np.arange(49), np.arange(49)] = True                  # claims every query selects itself: false for a permutation
    with pytest.raises(AssertionError):
        A.prove({"kind": "select", "q": q, "k": k, "win": win, "scale": 32.0 ** -0.5}, A.swin_extra(op["bias"], reg, C // 32, B))


# ================================================================================================ honest emulation
@pytest.mark.parametrize("kernel", KERNELS)
def test_honest_emulation_passes(kernel):
    v, cmp_ok = _verdicts(kernel, None)
    print(f"\n{kernel} honest emulation at {W.HOST_GEOM}: " +
          ", ".join(f"{n} {'exact' if i.get('nbad') == 0 else format(i.get('worst', float('nan')), '.3f')}" for n, i in v.items()))
    for n, i in v.items():
        assert i["ok"], (kernel, n, i)
    assert cmp_ok


# ================================================================================================ seeded defects
@pytest.mark.parametrize("kernel", KERNELS)
def test_every_defect_is_rejected_or_listed(kernel):
    print(f"\n{kernel}: defect -> instruments that reject it | passes _cmp(1e-2)")
    for d in W.DEFECTS:
        if not _applies(kernel, d):
            print(f"  {d:24s} n/a (one window per workgroup)")
            continue
        v, cmp_ok = _verdicts(kernel, d)
        rej = [n for n, i in v.items() if not i["ok"]]
        note = ""
        if not rej:
            note = "NOT REJECTED: " + (W.NOT_REJECTED.get(d) or W.NOT_REJECTED_AT.get((kernel, d), "?"))
        print(f"  {d:24s} {' '.join(rej) or '-':40s} cmp {'passes' if cmp_ok else 'fails'}  {note}")
        if d in W.NOT_REJECTED or (kernel, d) in W.NOT_REJECTED_AT:
            continue
        assert rej, f"{kernel}: no instrument rejects {d}"


@pytest.mark.parametrize("kernel", KERNELS)
def test_who_sees_what(kernel):
    """The claims of the instruments' docstring that the design rests on."""
    C = W.KERNELS[kernel][0]

    def rejected(d):
        return {n for n, i in _verdicts(kernel, d)[0].items() if not i["ok"]}
    assert "b" in rejected("head_cross") and "b" in rejected("swap_hw") and "b" in rejected("swap_shift")
    assert {"a-flat", "a-mask"} <= rejected("mask_region_off_by_one") and "b-soft" in rejected("scale_half") & rejected("scale_off")
    assert {"a-select", "a-tie"} <= rejected("unmasked_pad") and "b" not in rejected("unmasked_pad")
    assert {"a-select", "b"} <= rejected("v_key_order")
    assert {"a-select", "b"} <= rejected("roll_back_wrong") & rejected("res_rolled") & rejected("drop_proj_bias")
    assert "a-select" in rejected("drop_wbeta") and "a-tie" in rejected("no_half_exchange")
    if C < 384:
        assert {"a-select", "b"} <= rejected("c_minus_1")
    assert {"a-select", "b"} <= rejected("trunc_pack") & rejected("neighbour_stats")
    # what the old criterion lets through on Gaussian data
    for d in ("c_minus_1", "trunc_pack", "truncate_p", "scale_off", "unmasked_pad"):
        assert _verdicts(kernel, d)[1], f"{d}: _cmp(1e-2) was expected to pass it"
