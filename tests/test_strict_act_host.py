"""CPU proofs for tests/test_strict_act_gpu.py: the float32 emulations of tests/_strict.py (S.emulate with an activation,
S.emu_se_scale) go through the two instruments the GPU module uses -- bit equality on each activation's lattice, and the
per-element bound S.act_bound / S.se_ref plus the rounding bias on Gaussian operands.  The honest emulation passes both for every
activation; each seeded defect, one switch at a time, is rejected by at least one of them.  Figures (pytest -s) on a
520 x 64 x 72 GEMM with a residual, bf16 output; "cmp" = what `_cases._cmp(got, ref, 1e-2)` says of the same Gaussian output:

    defect            on                exact      bound      bias       cmp
    skip_tail_vec     every activation  rejects    rejects    rejects    rejects (the shift is wide here: the skipped values are large)
    act_before_res    every activation  rejects    rejects    rejects    rejects
    act_before_shift  every activation  rejects    rejects    rejects    rejects
    trunc             every activation  passes     rejects    rejects    PASSES   (ratio 1.98: up to one ulp; bias -0.39 .. -0.53)
    erf_gelu          gelu_tanh         passes     rejects    rejects    PASSES   (ratio 8.2, bias +0.081)
    pair_repeat       gelu_tanh         rejects    rejects    rejects    rejects
    no_clamp6         hard_swish        rejects    rejects    rejects    rejects

(the last column is asserted below: `EXPECT_CMP_PASSES`).  se_scale: `lost_lane` and
`w2_untransposed` are rejected by both instruments on (96, 33, 343) and (1032, 6, 67).
Worst |err| / bound of the honest emulations: printed; recorded in tests/test_strict_act_gpu.py next to the MI355X's.
"""
import numpy as np
import pytest

from tests import _strict as S
from tests import _strict_lngemm as G

ACTS = ["gelu_tanh", "hard_swish", "hard_sigmoid", "sigmoid", "silu"]
M, KR, NO = 520, 64, 72
DEFECTS = {"skip_tail_vec": ACTS, "act_before_res": ACTS, "act_before_shift": ACTS, "trunc": ACTS, "erf_gelu": ["gelu_tanh"],
           "pair_repeat": ["gelu_tanh"], "no_clamp6": ["hard_swish"]}
# (defect, activation) pairs whose Gaussian output the former check `_cmp(got, ref, 1e-2)` lets through
EXPECT_CMP_PASSES = {("trunc", a) for a in ACTS} | {("erf_gelu", "gelu_tanh")}


def _data(mode, act, out="bf16"):
    """The operands of tests/_strict_gpu.py's runners, at GEMM size: (x, w, sc, sh, r, ref, bound or None)."""
    rng = S.rng_of(900 + S.ACT_CODES[act])
    step = S.LATTICE_STEP[act]
    if mode == "int":
        hard = step == 3
        x = S.int_tensor(rng, (M, KR), 1 if hard else 2)
        w = S.pm1_rows(rng, NO, KR, 32)
        sc = S.int_scale(rng, NO) * np.float32(step)
        sh = S.int_tensor(rng, (NO,), 4 if hard else 8) * np.float32(step)
        r = S.int_tensor(rng, (M, NO), 4 if hard else 16) * np.float32(step)
        _, mag, p = S.gemm_ref(x, w, sc, sh, r, act, pre=True)
        return x, w, sc, sh, r, S.prove_lattice(f"host/{act}", p, mag, act, [w], stored=[x, w, r], out=out), None
    x, w = S.bf(rng.standard_normal((M, KR))), S.bf(rng.standard_normal((NO, KR)) / np.sqrt(KR))
    sc, sh = S.gauss_scale(rng, NO), (4.0 * rng.standard_normal(NO)).astype(np.float32)
    r = S.bf(rng.standard_normal((M, NO)))
    _, mag, p = S.gemm_ref(x, w, sc, sh, r, act, pre=True)
    S.prove_reach(f"host/{act}", p, act)
    ref, bound = S.act_bound(p, mag, KR, act, out)
    return x, w, sc, sh, r, ref, bound


def _run(act, defect=None, out="bf16"):
    """(exact ok, bound info, bias info, passes the former check)."""
    kw = {} if defect is None else ({"store": "trunc"} if defect == "trunc" else {defect: True})
    x, w, sc, sh, r, ref, _ = _data("int", act, out)
    e = S.check_exact(S.emulate(x, w, sc, sh, r, act, out=out, **kw), ref)
    x, w, sc, sh, r, ref, bound = _data("gauss", act, out)
    y = S.emulate(x, w, sc, sh, r, act, out=out, **kw)
    a = S.check_bound(y, ref, None, 0, out, bound=bound)
    applies = out == "bf16" and int((np.abs(ref) >= 2.0 ** -6).sum()) >= S.BIAS_MIN_ELEMS
    b = S.check_bias(y, ref, out) if applies else {"ok": True, "bias": float("nan"), "n_bias": 0}
    return e["ok"], a, b, G.cmp_1e2(y, ref)


@pytest.mark.parametrize("out", ["bf16", "fp32"])
@pytest.mark.parametrize("act", ACTS + ["none", "relu"])
def test_honest_emulation_passes(act, out):
    if act in ("none", "relu"):                         # the bound reduces to elem_bound: today's cases are unchanged
        x, w, sc, sh, r, ref, _ = _data("gauss", "gelu_tanh", out)
        ref, mag, p = S.gemm_ref(x, w, sc, sh, r, act, pre=True)
        ref2, bound = S.act_bound(p, mag, KR, act, out)
        assert np.array_equal(ref, ref2) and np.array_equal(bound, S.elem_bound(ref, mag, KR, out))
        return
    exact, a, b, cmp_ok = _run(act, None, out)
    print(f"{act}/{out}: lattice exact {exact} | worst |err|/bound {a['worst']:.3f} over {a['n']} | bias {b['bias']:+.4f} over {b['n_bias']} | cmp {cmp_ok}")
    assert exact and a["ok"] and b["ok"] and cmp_ok, (act, a, b)


@pytest.mark.parametrize("defect,act", [(d, a) for d, acts in DEFECTS.items() for a in acts])
def test_defect_is_rejected(defect, act):
    exact, a, b, cmp_ok = _run(act, defect)
    seen = [n for n, ok in (("exact", exact), ("bound", a["ok"]), ("bias", b["ok"])) if not ok]
    print(f"{defect}/{act}: rejected by {seen or 'NOTHING'} (worst ratio {a['worst']:.2f}, bias {b['bias']:+.3f}) | the former check {'passes' if cmp_ok else 'rejects'} it")
    assert seen, f"{defect}/{act} passes both instruments"
    assert cmp_ok == ((defect, act) in EXPECT_CMP_PASSES), f"{defect}/{act}: the former check says {cmp_ok}"


def test_lattice_claims_hold_for_act32():
    """|k| <= 256 lattice steps: the float32 emulation equals the lattice function bit for bit, and act64 rounds to it."""
    for act in ACTS:
        step = S.LATTICE_STEP[act]
        v = (np.arange(-256, 257) * step).astype(np.float32)
        lat = S.lattice_value(v, act)
        assert np.array_equal(S.act32(v, act).astype(np.float64), lat), act
        assert np.array_equal(S.act32(v, act).astype(np.float64) == 0, lat == 0), act
        assert np.array_equal(np.asarray(S.act64(v, act), np.float32).astype(np.float64), lat), act
        assert 0 < np.abs(S.act64(v, act) - lat).max() < 1e-50 or act.startswith("hard"), act
    assert np.float64(np.float32(1) / np.float32(6)) == (1.0 + 2.0 ** -25) / 6.0 or abs(np.float64(np.float32(1) / np.float32(6)) * 6 - 1 - 2.0 ** -25) < 2.0 ** -50


def test_lipschitz_constants():
    for act, want in (("hard_swish", 1.5), ("hard_sigmoid", 1 / 6), ("sigmoid", 0.25), ("silu", 1.0998), ("gelu_tanh", 1.1290)):
        L = S.act_lipschitz(act)
        print(f"L({act}) = {L:.6f}")
        assert want - 1e-6 <= L <= want + 1e-3, (act, L)
    assert S.act_lipschitz("none") == 1.0 and S.act_lipschitz("relu") == 1.0


def test_prove_lattice_refuses_bad_data():
    x, w, sc, sh, r, ref, _ = _data("int", "hard_swish")
    _, mag, p = S.gemm_ref(x, w, sc, sh, r, "hard_swish", pre=True)
    with pytest.raises(AssertionError, match="leaves the lattice"):
        S.prove_lattice("off", p + 1.0, mag, "hard_swish", [w])
    with pytest.raises(AssertionError, match="not exact in bf16"):
        S.prove_lattice("big", 3 * p, 3 * mag, "hard_swish", [w])
    with pytest.raises(AssertionError, match="negative"):
        S.prove_lattice("signs", np.abs(p), mag, "hard_swish", [w])


# ------------------------------------------------------------------------------------------------ se_scale
SE_CASES = [(C, Sq, HW, a1, a2, bias) for (C, Sq, HW) in S.SE_SHAPES for (a1, a2) in S.SE_ACTS for bias in (True, False)]


@pytest.mark.parametrize("C,Sq,HW,a1,a2,bias", SE_CASES, ids=[f"{c[0]}_{c[1]}_{c[2]}_{c[3]}_{c[4]}_{'bias' if c[5] else 'nobias'}" for c in SE_CASES])
def test_se_honest_emulation_passes(C, Sq, HW, a1, a2, bias):
    ops = S.se_data("int", C, Sq, HW, a1, a2, bias)
    ref = S.se_prove_exact("se", *ops, a1, a2)
    e = S.check_exact(S.emu_se_scale(*ops, a1, a2), ref)
    ops = S.se_data("gauss", C, Sq, HW, a1, a2, bias)
    f = S.se_ref(*ops, a1, a2)
    a = S.check_bound(S.emu_se_scale(*ops, a1, a2), f["ref"], None, 0, "bf16", bound=f["bound"])
    print(f"se_scale {C}_{Sq}_{HW} {a1}/{a2} bias {bias}: exact {e['ok']} | worst |err|/bound {a['worst']:.3f} over {a['n']}")
    assert e["ok"] and a["ok"], (e, a)


@pytest.mark.parametrize("defect", ["lost_lane", "w2_untransposed", "trunc"])
@pytest.mark.parametrize("C,Sq,HW", [(96, 33, 343), (1032, 6, 67)])
def test_se_defect_is_rejected(C, Sq, HW, defect):
    kw = {"store_mode": "trunc"} if defect == "trunc" else {defect: True}
    seen, cmp_pass = [], []
    for a1, a2 in S.SE_ACTS:
        ops = S.se_data("int", C, Sq, HW, a1, a2, True)
        ref = S.se_prove_exact("se", *ops, a1, a2)
        if not S.check_exact(S.emu_se_scale(*ops, a1, a2, **kw), ref)["ok"]:
            seen.append(f"exact {a1}/{a2}")
        ops = S.se_data("gauss", C, Sq, HW, a1, a2, True)
        f = S.se_ref(*ops, a1, a2)
        y = S.emu_se_scale(*ops, a1, a2, **kw)
        if not S.check_bound(y, f["ref"], None, 0, "bf16", bound=f["bound"])["ok"]:
            seen.append(f"bound {a1}/{a2}")
        cmp_pass.append(G.cmp_1e2(y, f["ref"]))
    print(f"se_scale {C}_{Sq}_{HW} {defect}: rejected by {seen or 'NOTHING'} | the former check passes {sum(cmp_pass)} of {len(cmp_pass)}")
    if defect == "trunc":                  # 3 x C < 4096 outputs: no bias verdict, and a truncated store stays within one ulp -- on record
        return
    assert any(s.startswith("exact") for s in seen) and any(s.startswith("bound") for s in seen), seen
