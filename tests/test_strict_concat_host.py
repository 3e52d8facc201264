"""CPU proofs for tests/test_strict_concat_gpu.py: the float32 emulations of tests/_strict_concat.py (each kernel's order of
operations, the 3x3 ones decoding the PACKED fragments by the layout csrc/flat3x3.h states) go through the instruments the GPU module
uses, on the data the GPU module uses.  The honest emulation passes at every case and mode; each seeded defect, one switch at a
time, is rejected at the shapes of C.REJECTED_AT by at least one instrument (exact, rounding-visible exact, bound, bias, sentinel /
guard); where a defect is NOT rejected, and why, is stated in tests/_strict_concat.py's docstring and asserted here
(halo_not_zero_past_M; swap_rs on 1 x 1 maps; shift_from at N = 16; read_past_C with NaN alone; round_before_mean in the
three general modes).  The worst |err| / bound of the honest emulations is printed (-s) and recorded in that docstring."""
import numpy as np
import pytest

from eqxvision_amd import ops
from tests import _strict as S
from tests import _strict_concat as C

KERNELS = list(C.CASES)
ALL = [(k, i) for k in KERNELS for i in range(len(C.CASES[k]))]
_seen = set()


def _ids(v):
    return f"{v[0]}{v[1]}" if isinstance(v, tuple) else str(v)


def _run(kernel, case, mode, defect=None, arg=None):
    d = C.DATA[kernel](case, mode)
    return C.verdict(d, C.EMU[kernel](d, defect, arg), mode)


# ================================================================================================ the packers
@pytest.mark.parametrize("N,S_,s_pad", [(32, 16, None), (64, 48, None), (16, 16, None), (48, 32, None), (80, 24, 32), (48, 5, 16), (144, 128, None)])
def test_fragments_follow_the_documented_layout(N, S_, s_pad):
    """decode(pack(w)) == w for a plain KRSC filter of distinct values; the rows up to a multiple of 32 and the channels up to
    s_pad are zeros; tile t of a filter is entry t of the array, i.e. 9 KC * 64 uint4 behind tile t - 1."""
    rng = S.rng_of(N * 1000 + S_)
    w = S.bf(rng.permutation(N * 9 * S_).reshape(N, 3, 3, S_) % 251 - 125.0)
    f = C.pack3x3(w, s_pad)
    Sp = S_ if s_pad is None else s_pad
    assert f.shape == (-(-N // 32), 9 * Sp // 16, 64, 8)
    back = C.decode_fragments(f, 9).reshape(-1, 3, 3, Sp)
    assert np.array_equal(back[:N, :, :, :S_], w)
    assert not back[N:].any() and not back[:, :, :, S_:].any()
    assert [C.tile_row(p) for p in range(32)] == list(ops.FIRE_TILE_ROW)
    if N % 32 == 0 and s_pad is None:                                   # fire_fragments itself: 1x1 and 3x3
        krsc = lambda a: np.ascontiguousarray(a.transpose(0, 3, 1, 2))
        assert np.array_equal(ops.fire_fragments(krsc(w)), f)
        w1 = w[:, 1:2, 1:2]
        assert np.array_equal(C.decode_fragments(ops.fire_fragments(krsc(w1)), 1), w1.reshape(N, 1, S_))


def test_case_tables_reach_what_the_issue_lists():
    maps = set(C.MAPS)
    for k in ("slice", "pair", "fire"):
        assert {c[:3] for c in C.CASES[k]} == maps, k
    sl = C.SLICE_CASES
    assert {c[3] for c in sl} == {16, 48, 128} and {c[4] for c in sl} == {16, 32, 48, 80, 96, 144}
    assert any(c[5] for c in sl) and any(c[6] > 0 for c in sl)
    for c in sl + [C.SLICE_EDGE]:                                       # room for upper_half_stored to land on the sentinel
        assert c[4] % 32 != 16 or c[6] + c[4] + 16 <= c[7]
    pa = C.PAIR_CASES
    assert {c[3] for c in pa} >= {(16, 48), (48, 16), (128, 16)} and {c[4] for c in pa} >= {(16, 16), (80, 48), (96, 144)}
    assert any(c[5][1] < c[5][0] for c in pa) and any(c[7][1] < c[7][0] for c in pa)
    for c in pa:
        own = np.zeros(c[6], bool)
        for i in range(2):
            own[c[5][i]:c[5][i] + c[3][i]] = True
        assert not own.all(), "no channel of t is left for the NaN"
    fi = C.FIRE_CASES
    assert {c[3] for c in fi} == {16, 32, 48, 64} and {c[4] for c in fi} == {64, 256} and any(c[5] for c in fi) and any(c[6] for c in fi)
    sp = C.SPLIT_CASES
    assert {c[1] for c in sp} == {16, 64, 80, 128, 144} and {c[2] for c in sp} == {16, 48, 144, 272} and {c[0] for c in sp} == {1, 129, 257}
    assert {c[3] for c in sp} >= {16, 48, 128} and any(c[3] == c[2] - 16 for c in sp) and any(c[3] == c[2] for c in sp)
    assert any(c[4] > 0 for c in sp) and any(c[6] > 0 for c in sp) and any(c[3] < c[2] and c[5] != c[7] for c in sp)
    pr = C.PREACT_CASES
    assert {c[:3] for c in pr if c[3] == 2} == {(2, 2, 1), (3, 2, 2), (2, 3, 2), (5, 7, 2), (15, 14, 2)} and (1, 1, 1, 1) in {c[:4] for c in pr}
    assert {c[4] for c in pr} == {16, 64, 80, 128, 144} and {c[5] for c in pr} == {16, 48, 144, 272}
    assert {c[0] * c[1] * c[2] for c in pr if c[3] == 1} == {1, 129, 257}
    for pool in (1, 2):
        assert {c[6] for c in pr if c[3] == pool} == {True, False}
    assert all(c[8] == 0 for c in pr if c[6]) and all(c[8] > 0 for c in pr if not c[6]) and sum(c[7] == 16 for c in pr) >= 10


def test_slice_gate_edge_from_the_lds_formula():
    """S = 512, W = 13 is the largest range the 160 KB gate admits; W = 14 is refused (the GPU module asserts the entry's answer)."""
    assert C.flat_lds_bytes(128, 13, 512) == 157 * 1040 <= C.FLAT_LDS_MAX < C.flat_lds_bytes(128, 14, 512)
    assert C.SLICE_EDGE[:2] == (2, 13) and C.SLICE_EDGE[3] == 512
    assert 9 * 512 > S.BIAS_MAX_KRED                                    # the bound only


# ================================================================================================ honest emulations
@pytest.mark.parametrize("mode", ["int", "gauss"])
@pytest.mark.parametrize("kernel,i", ALL, ids=_ids)
def test_honest_emulation_passes(kernel, i, mode):
    v = _run(kernel, C.CASES[kernel][i], mode)
    print(f"{kernel}/{C.case_id(C.CASES[kernel][i])}/{mode}: worst |err|/bound {v['worst']:.3f}, bias {v['bias']}, wrong {v['wrong']}")
    assert v["ok"], v["why"]


def test_worst_ratio_per_kernel():
    for k in KERNELS:
        worst = max(_run(k, c, "gauss")["worst"] for c in C.CASES[k])
        print(f"{k}: worst |err| / bound of the honest emulation over its Gaussian cases: {worst:.3f}")
        assert worst <= 1.0, f"{k}: the count of roundings is wrong (recount from the source; no factor)"
    v = _run("slice", C.SLICE_EDGE, "gauss")
    assert v["ok"] and not v["bias"], v


@pytest.mark.parametrize("kernel", KERNELS)
def test_a_gaussian_case_is_bias_eligible(kernel):
    """After ReLU has zeroed about half the outputs, at least one Gaussian case per kernel still has 4096 elements at |ref| >= 2^-6 in
    EVERY slice with kred <= 1152, so the bias rule runs at every kernel."""
    n = 0
    for c in C.CASES[kernel]:
        d = C.DATA[kernel](c, "gauss")
        n += all(C.bias_applies(ref, kr) for (_, _, ref, _), kr in zip(d["slices"], d["kred"]))
    assert n >= 1


# ================================================================================================ rounding-visible exact
@pytest.mark.parametrize("kernel", KERNELS)
def test_round_cases(kernel):
    """The preconditions (ties >= 10 %, truncation-visible >= 25 %) are asserted inside the builder, on the reference alone."""
    case = C.ROUND[kernel]
    assert _run(kernel, case, "round")["ok"]
    for mutant in C.STORE_DEFECTS:
        v = _run(kernel, case, "round", mutant)
        assert not v["ok"] and v["wrong"] > 0, (kernel, mutant)
        _seen.add(mutant)
    d = C.DATA[kernel](case, "round")
    if kernel in ("slice", "preact"):
        assert (d["slices"][0][2] < 0).any(), "the identity store sees no negative value"


@pytest.mark.parametrize("kernel", KERNELS)
def test_truncation_fails_the_bias_rule(kernel):
    hit = 0
    for c in C.CASES[kernel]:
        d = C.DATA[kernel](c, "gauss")
        if all(C.bias_applies(ref, kr) for (_, _, ref, _), kr in zip(d["slices"], d["kred"])):
            v = C.verdict(d, C.EMU[kernel](d, "trunc"), "gauss")
            assert any("bias" in w for w in v["why"]), (kernel, c, v["why"])
            hit += 1
    assert hit


# ================================================================================================ seeded defects
PAIRS = [(d, k, i, a) for d, where in C.REJECTED_AT.items() for k, i, a in where]


@pytest.mark.parametrize("defect,kernel,i,arg", PAIRS, ids=_ids)
def test_defect_is_rejected(defect, kernel, i, arg):
    case = C.CASES[kernel][i]
    res = {m: _run(kernel, case, m, defect, arg) for m in ("int", "gauss")}
    print(f"{defect} @ {kernel}/{C.case_id(case)}: " + ", ".join(f"{m} {'REJECTED' if not v['ok'] else 'passes'}" for m, v in res.items()))
    assert not res["int"]["ok"] or not res["gauss"]["ok"]
    if defect in ("upper_half_stored", "dead_wave_stores", "n0_group_to_dst0"):
        assert all(any("outside the slices" in w or "guard" in w for w in v["why"]) for v in res.values()), "the sentinel has to see it"
    _seen.add(defect)


def test_round_before_mean_needs_its_own_case():
    for i, c in enumerate(C.PREACT_CASES):
        if c[3] == 2:
            assert _run("preact", c, "int", "round_before_mean")["ok"] and _run("preact", c, "gauss", "round_before_mean")["ok"]
    d = C.preact_mean_case()
    assert C.verdict(d, C.emu_preact(d), "int")["ok"]
    v = C.verdict(d, C.emu_preact(d, "round_before_mean"), "int")
    assert not v["ok"] and v["wrong"] == d["slices"][0][2].size          # every output is two off
    _seen.add("round_before_mean")


def test_where_a_defect_is_not_rejected():
    for k, cases in (("slice", C.SLICE_CASES), ("pair", C.PAIR_CASES), ("fire", C.FIRE_CASES)):
        for c in cases:
            d = C.DATA[k](c, "int")
            honest, mutant = C.EMU[k](d), C.EMU[k](d, "halo_not_zero_past_M")
            assert all(np.array_equal(a, b) for a, b in zip(honest, mutant))
    assert _run("slice", C.SLICE_CASES[0], "int", "swap_rs")["ok"]                    # 1 x 1 maps: the centre tap alone
    assert _run("slice", C.SLICE_CASES[0], "int", "drop_kstep", (0, 0))["ok"]
    assert _run("slice", C.SLICE_CASES[1], "int", "last_prefetch_repeat")["ok"]       # H = 1: taps (2, .) are outside
    assert _run("split", C.SPLIT_CASES[0], "int", "shift_from")["ok"]                 # N = 16: the roll is the identity
    assert _run("slice", C.SLICE_CASES[4], "int", "neighbour_image")["ok"]            # B = 1, M = one tile: nothing next to it
    d = C.preact_data(C.PREACT_CASES[2], "int")                                       # NaN alone is laundered three times over
    assert C.verdict(d, C.emu_preact(d, "read_past_C", poison_nan_only=True), "int")["ok"]
    assert not C.verdict(d, C.emu_preact(d, "read_past_C"), "int")["ok"]


def test_zz_every_listed_defect_is_accounted_for():
    """Runs last in this module: the defects rejected above and those listed with a reason make up the issue's list."""
    expect = set(C.ISSUE_DEFECTS) | {"half_up"}
    assert set(C.REJECTED_AT) | set(C.STORE_DEFECTS) | set(C.SPECIAL) | set(C.NOT_REJECTED) == expect
    assert _seen == expect - set(C.NOT_REJECTED), sorted(expect - set(C.NOT_REJECTED) - _seen)
