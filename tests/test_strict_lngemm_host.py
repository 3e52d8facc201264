"""CPU proofs for tests/test_strict_lngemm_gpu.py: the float32 emulations of tests/_strict_lngemm.py (each kernel's order of
operations) go through the two instruments the GPU module uses.  The honest emulation passes both at every kernel; each seeded
defect, one switch at a time, is rejected by at least one of them:

    neighbour_stats   the statistics of row m ^ 1                      exact (neighbours differ by >= 4 in a_r) and bound
    c_minus_1         variance divided by C - 1                        exact: +-1 becomes 0.9961 at C = 96 / 192; the midpoint rows at 192 / 384
    no_eps            eps omitted                                      bound: the constant row (0 * rsqrt(0), or a rounding residue
                                                                       blown up by rsqrt of a residue); the exact rows cannot see it
    drop_wbeta        W . beta missing from the folded bias >= 128     exact, bound
    drop_chunk        one 16-wide k-step not accumulated               exact, bound
    swap_hidden       two hidden units trade places in W2              exact, bound at C = 96
    res_prev_row      the last ragged tile adds the residual of m - 1  exact, bound
    trunc_pack        truncation instead of RNE at the bf16 packs      exact where a^2 is small enough for eps to show, the bias rule
                                                                       where the output is bf16

At C = 384 the factor sqrt(383 / 384) = 0.9987 moves no +-1 fragment value off 1.0 in bf16; the streamed kernels therefore also
run the exact chain on MIDPOINT rows (tests/_strict_lngemm.py, instrument 1b), whose normalised values sit just above a bf16 rounding
midpoint, and "exact" below means both exact cases for them.
The figures (worst |err| / bound of the honest emulation, and which defects `_cmp(got, ref, 1e-2)` lets through) are printed (-s)
and recorded in tests/_strict_lngemm.py's docstring.
"""
import numpy as np
import pytest

from tests import _strict as S
from tests import _strict_lngemm as G
from tests import _strict_norm as N

# kernel -> (kind, args): the smallest case with a ragged last tile
LINEAR = {"ln_linear_k96": (8192 + 5, 96, 200, "fp32"), "ln_linear_k192": (8192 + 5, 192, 200, "bf16")}
MLP = {"ln_mlp96_f32": (1055, 96, "fp32", False, "half"), "ln_mlp96_bf16": (1055, 96, "bf16", False, "half"),
       "ln_mlp96_res_f32in": (1055, 96, "fp32", True, "half"), "ln_mlp96_res_bf16in": (1055, 96, "bf16", True, "half"),
       "ln_mlp_stream_c192": (133, 192, "fp32", False, "stream"), "ln_mlp_stream_c192_res": (133, 192, "fp32", True, "stream"),
       "ln_mlp_stream_c384": (197, 384, "fp32", False, "stream"), "ln_mlp_stream_c384_res": (197, 384, "fp32", True, "stream")}


def _linear(name, defect):
    """(exact ok, bound info, bias info, passes _cmp at 1e-2)."""
    M, K, N_, st = LINEAR[name]
    x, wf, bfold, b, ref = G.linear_exact(M, K, N_, st, 1)
    e = S.check_exact(G.emu_ln_linear(x, wf, bfold, b, 1, defect=defect), ref)
    xg, wg, bg, b0, refg, boundg = G.linear_gauss(M, K, N_, st, 2)
    y = G.emu_ln_linear(xg, wg, bg, b0, 2, defect=defect)
    a, bias = N.judge(y, refg, boundg, "bf16")
    return e["ok"], a, bias, G.cmp_1e2(y, refg)


def _mlp(name, defect):
    M, C, st, res, kind = MLP[name]
    x, r, w1f, b1f, b1, w2, b2, ref, out = G.mlp_exact(M, C, st, res)
    e = S.check_exact(G.emu_ln_mlp(x, r, w1f, b1f, b1, w2, b2, out, kind, defect=defect), ref)
    xg, rg, w1g, b1g, b10, w2g, b2g, refg, boundg, out = G.mlp_gauss(M, C, st, res)
    y = G.emu_ln_mlp(xg, rg, w1g, b1g, b10, w2g, b2g, out, kind, defect=defect)
    a, bias = N.judge(y, refg, boundg, out)
    exact = e["ok"]
    if kind == "stream":                                         # the streamed kernels have the midpoint rows as well
        x, r, w1f, b1f, w2, b2, ref = G.mlp_midpoint(M, C, res)
        exact = exact and S.check_exact(G.emu_ln_mlp(x, r, w1f, b1f, b1f, w2, b2, "fp32", kind, defect=defect), ref)["ok"]
    return exact, a, bias, G.cmp_1e2(y, refg)


def _run(name, defect):
    return _linear(name, defect) if name in LINEAR else _mlp(name, defect)


PAIRS = [(k, d) for k in LINEAR for d in G.LINEAR_DEFECTS] + [(k, d) for k in MLP for d in G.DEFECTS]


# ================================================================================================ tables and constants
def test_case_tables_reach_what_they_claim():
    # ln_linear: every wave has at most one tile at the gate shapes; at LINEAR_M2 wave 0 walks to tile 2048, the ragged one
    for M, K, N_, _, _ in G.LINEAR_CASES:
        assert M >= G.LINEAR_MIN_M and N_ % 8 == 0 and N_ > 64
    gx, gy, npass, waves, tiles = G.linear_grid(8192 + 5, 96, 200)
    assert (gy, npass) == (1, 2) and tiles <= waves
    gx, gy, npass, waves, tiles = G.linear_grid(G.LINEAR_M2, 96, 200)
    assert (gx, waves, tiles) == (256, 2048, 2049) and G.LINEAR_M2 % 32 == 5
    assert G.linear_grid(G.LINEAR_M2 - 32, 96, 200)[4] == 2048                       # one tile fewer: nobody walks
    assert G.linear_grid(8192 + 5, 192, 256)[1:3] == (2, 1)                          # K = 192: one slab per block, two block columns
    # ln_mlp96: 12 waves x 256 blocks; 8 waves with the flag
    assert G.mlp_grid(G.MLP_M2) == (256, 3072, 3073) and G.mlp_grid(G.MLP_M2 - 32)[2] == 3072
    assert G.mlp_grid(G.MLP_M2_W8, 8) == (256, 2048, 2049)
    for M, _, _, _ in G.MLP96_CASES:
        assert M >= G.MLP_MIN_M
    assert {M % 32 for M, _, _, _ in G.MLP96_CASES} == {0, 1, 31, 5} | {1057 % 32}
    # ln_mlp_stream: one block per tile of 128 (C = 192) / 64 (C = 384) rows: one tile or two, a ragged tail, a third block
    for M, C, _ in G.STREAM_CASES:
        assert M >= G.STREAM_MIN_M
    assert sorted({-(-M // 128) for M, C, _ in G.STREAM_CASES if C == 192}) == [1, 2, 3]
    assert sorted({-(-M // 64) for M, C, _ in G.STREAM_CASES if C == 384}) == [2, 3, 4]


def test_gelu_constants():
    t = G.gelu_exact_from()
    assert 10.0 < t < 10.1                                       # "a little above 10": multiples of 16 are far beyond it
    # in float32 emulation: exact ReLU on multiples of 16, 0 at 0 (sign of zero aside)
    x = np.arange(-4096.0, 4096.0 + 16.0, 16.0, dtype=np.float32)
    assert np.array_equal(S.act32(x, "gelu_tanh"), np.maximum(x, 0.0))
    L = G.gelu_lipschitz()
    assert 1.128 < L < 1.130                                     # max gelu' = 1.1289...; the value used is the computed one


@pytest.mark.parametrize("stream,mult16,C", [("fp32", False, 96), ("bf16", False, 192), ("bf16", True, 96), ("fp32", False, 384)])
def test_pm1_rows_are_proved(stream, mult16, C):
    x, sg, a, m = G.pm1_rows_x(133, C, stream, 7, mult16)
    dev, total = G.prove_pm1("pm1", x, sg, a, m)
    assert dev < 2.0 ** -10 and total < 2.0 ** -9
    for kind in ("half", "stream") if C % 12 == 0 and (C // 12) & (C // 12 - 1) == 0 else ("half",):
        assert np.array_equal(G._normalise(x, G.EPS, kind, None), sg)            # the emulated fragment IS +-1
    # a row that breaks the construction is refused: a_r equal to its neighbour's
    a2 = a.copy()
    a2[1] = a2[0]
    with pytest.raises(AssertionError):
        G.prove_pm1("pm1", (m[:, None] + a2[:, None] * sg).astype(np.float32), sg, a2, m)


# ================================================================================================ honest emulations pass
@pytest.mark.parametrize("name", list(LINEAR) + list(MLP))
def test_honest_emulation_passes(name):
    exact, a, bias, cmp_ok = _run(name, None)
    print(f"{name}: exact {exact}, worst |err|/bound {a['worst']:.3f}, bias {bias['bias']:+.4f} over {bias['n_bias']}")
    assert exact and a["ok"] and bias["ok"] and cmp_ok, (exact, a, bias)


# ================================================================================================ every defect is rejected
@pytest.mark.parametrize("name,defect", PAIRS, ids=lambda v: v)
def test_defect_is_rejected(name, defect):
    exact, a, bias, cmp_ok = _run(name, defect)
    print(f"{name}/{defect}: exact {exact}, bound {a['ok']} (worst {a.get('worst', float('nan')):.3g}), bias {bias['ok']}, "
          f"_cmp(1e-2) {'lets it through' if cmp_ok else 'rejects it'}")
    assert not (exact and a["ok"] and bias["ok"])


@pytest.mark.parametrize("C", [192, 384])
def test_midpoint_rows_see_the_variance_divisor(C):
    """sqrt(383 / 384) = 0.99870 > 0.99805, the midpoint between 1 and the bf16 value below it: the +-1 fragment does not move at
    C = 384.  The midpoint rows are chosen so that it does: proved in float64 (prove_midpoint), and shown on the emulated fragment."""
    assert np.sqrt(383.0 / 384.0) > 1.0 - 2.0 ** -9 > np.sqrt(191.0 / 192.0) > np.sqrt(95.0 / 96.0)
    x, sg, a, m = G.pm1_rows_x(133, C, "fp32", 7)
    assert np.array_equal(G._normalise(x, G.EPS, "stream", "c_minus_1"), sg) == (C == 384)
    x, ks, plus = G.midpoint_rows_x(133, C, 7)
    assert len(set(ks)) == 4 and (plus.sum(1) == ks).all()
    frag = G.prove_midpoint("midpoint", x)
    assert np.array_equal(G._normalise(x, G.EPS, "stream", None), frag)
    assert (G._normalise(x, G.EPS, "stream", "c_minus_1") != frag).mean() > 0.25


def test_what_the_former_check_lets_through():
    """`_cmp(got, ref, 1e-2)` on the same Gaussian data: it passes these defects (printed per kernel); both new regimes together pass none of them."""
    passed = {}
    for name, defect in PAIRS:
        if _run(name, defect)[3]:
            passed.setdefault(defect, []).append(name)
    for d, ks in passed.items():
        print(f"_cmp(1e-2) lets {d} through at: {', '.join(ks)}")
    assert {"c_minus_1", "trunc_pack", "swap_hidden", "drop_wbeta"} <= set(passed)
    assert "neighbour_stats" not in passed


# ================================================================================================ mv_cnblock_dw_fwd: the two exact cases
@pytest.mark.parametrize("C", [96, 192])
def test_cnblock_exact_cases(C):
    """The emulation passes both; a dropped tap fails both; the neighbouring pixel's statistics, C - 1 and the truncating pack fail
    the sign case (eps cannot show on integers: |v| >= 1)."""
    assert (G.cnb_tile(96), G.cnb_tile(192)) == (32, 16) and G.cnb_shape(C)[2] % G.cnb_tile(C) == 5
    x, w, bias, ref = G.cnb_exact(C)
    assert S.check_exact(G.emu_cnblock(x, w, bias, 0, "bf16"), ref)["ok"]
    assert not S.check_exact(G.emu_cnblock(x, w, bias, 0, "bf16", defect="drop_tap"), ref)["ok"]
    x, w, ref, keep = G.cnb_sign(C)
    assert S.check_exact(G.emu_cnblock(x, w, None, 1, "bf16")[keep], ref[keep])["ok"]
    for d in ("neighbour_stats", "c_minus_1", "drop_tap", "trunc_pack"):
        assert not S.check_exact(G.emu_cnblock(x, w, None, 1, "bf16", defect=d)[keep], ref[keep])["ok"], d


@pytest.mark.parametrize("C,xdt", G.CNB_CASES)
def test_cnblock_ln_bound(C, xdt):
    """normalize = 1 on Gaussian maps: the emulation is inside the bound and the bias rule; the neighbouring pixel's statistics, a
    dropped tap and the variance over C - 1 are outside the bound, the truncating store outside the bound and the bias rule."""
    x, w, bias, ref, bound = G.cnb_gauss(C, xdt)
    a, b = N.judge(G.emu_cnblock(x, w, bias, 1, "bf16"), ref, bound, "bf16")
    print(f"cnblock_ln C{C} {xdt}: worst |err|/bound {a['worst']:.3f}, bias {b['bias']:+.4f} over {b['n_bias']}")
    assert a["ok"] and b["ok"], (a, b)
    # no_eps is not seeded here: the Gaussian map has no pixel whose channel variance comes near eps = 1e-5 (the smallest is ~0.5),
    # and the sign case's |v| >= 1 neither: no test of this module can see eps in cnblock
    for d in ("neighbour_stats", "drop_tap", "trunc_pack", "c_minus_1"):
        a, b = N.judge(G.emu_cnblock(x, w, bias, 1, "bf16", defect=d), ref, bound, "bf16")
        print(f"   {d}: bound {a['ok']} (worst {a['worst']:.3g}), bias {b['ok']} ({b['bias']:+.4f})")
        assert not (a["ok"] and b["ok"]), d


@pytest.mark.parametrize("B,H,K,split", G.PATCH4_CASES)
def test_patch4_ln_bound(B, H, K, split):
    """mv_patch4_ln_fwd: the emulation is inside the bound at every case and each defect is outside it -- at the one-tile cases
    (H = 8: four tokens) too, where token 0 is the black patch that shows a missing eps."""
    x, hi, lo, b, g, be, ref, bound = G.patch4_gauss(B, H, K, split)
    assert ref.shape[0] == B * (H // 4) ** 2 and (H > 8) == (ref.shape[0] % 128 != 0 and ref.shape[0] > 128)
    a = S.check_bound(G.emu_patch4_ln(x, hi, lo, b, g, be, split), ref, None, 0, "fp32", bound=bound)
    print(f"patch4_ln B{B} H{H} K{K} split{int(split)}: worst |err|/bound {a['worst']:.3f}")
    assert a["ok"], a
    for d in ("neighbour_stats", "c_minus_1", "no_eps", "drop_chunk", "trunc_pack"):
        a = S.check_bound(G.emu_patch4_ln(x, hi, lo, b, g, be, split, defect=d), ref, None, 0, "fp32", bound=bound)
        print(f"   {d}: bound {a['ok']} (worst {a.get('worst', float('nan')):.3g})")
        assert not a["ok"], d


# ================================================================================================ mv_linear_lnout_fwd -> mv_linear_lnin_fwd
def _lnout_ok(info):
    return all(i["ok"] for i in info.values())


@pytest.mark.parametrize("case", G.LNFOLD_CASES, ids=G.lnfold_id)
def test_lnfold_pair(case):
    """The producer's emulation passes the five per-element / per-row checks and each producer defect fails one; the consumer's
    emulation, fed the producer's planes, is inside lnin_ref_bound and the bias rule, and each consumer defect is outside."""
    M, D, Kp, N2, act, row_mean = case
    x, w, b, res, wf, cs, bfold = G.lnfold_data(*case)
    y_ref, e_y = G.lnout_ref(*case)
    hi, lo, st = G.emu_lnout(x, w, b, res)
    info = G.check_lnout(hi, lo, st, y_ref, e_y)
    print(G.lnfold_id(case), {k: round(v["worst"], 4) for k, v in info.items()})
    assert _lnout_ok(info), info
    for d in G.LNOUT_DEFECTS:
        bad = G.check_lnout(*G.emu_lnout(x, w, b, res, defect=d), y_ref, e_y)
        print(f"   lnout {d}: fails {[k for k, v in bad.items() if not v['ok']]}")
        assert not _lnout_ok(bad), d
    ref, bound = G.lnin_ref_bound(hi, lo, wf, cs, bfold, act)
    a, bias = N.judge(G.emu_lnin(hi, st, wf, cs, bfold, act), ref, bound, "bf16")
    print(f"   lnin: worst |err|/bound {a['worst']:.3f}, bias {bias['bias']:+.4f} over {bias['n_bias']}")
    assert a["ok"] and bias["ok"], (a, bias)
    for d in G.LNIN_DEFECTS:
        y = G.emu_lnin(hi, st, wf, cs, bfold, act, defect=d)
        a, bias = N.judge(y, ref, bound, "bf16")
        print(f"   lnin {d}: bound {a['ok']} (worst {a.get('worst', float('nan')):.3g}), bias {bias['ok']}, _cmp(1e-2) passes {G.cmp_1e2(y, ref)}")
        assert not (a["ok"] and bias["ok"]), d
