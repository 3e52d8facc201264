"""CPU proofs for tests/test_strict_norm_gpu.py: the float32 emulations of tests/_strict_norm.py (LayerNorm family, batch moments,
BatchNorm folds) go through the checkers the GPU module uses, at its cases.  The correct emulation passes the exact and the
per-element instrument at every case; each defect, one switch at a time, fails the case named next to it:

    LayerNorm    one-pass variance (offset4096); eps omitted (the constant rows: 0 * rsqrt(0)); eps outside the root (rows of sigma 0.01,
                 where eps is a tenth of the variance; generic C = 22);
                 divisor C - 1; a dead clamped chunk counted into the sum (nch 13, 65, ...); the previous sub-row's statistics
                 (nch 13 at M = 64 / WIDTH + 1 = 5); the clamped row group stored (the guard, same case); gamma / beta one chunk late;
                 the truncating bf16 store (the bias instrument); patch-merge segments 1 and 2 swapped
    moments      a tail row skipped, a row counted twice (37 x 2048: 13 rows per block, three unrolled trips and a tail of one);
                 a partial read beyond G (the NaN workspace); d squared before the shift is subtracted;
                 fmaxf removed from the single-pass variance (constant channels with run_var = 0)

Not a switch: `y_lo rounded from a value already rounded to bf16`.  Rounding to bf16 is idempotent -- bf16(bf16(y)) == bf16(y) for
every y, and the fp32 plane is y itself -- so no input makes that defect differ from rounding once; the GPU module's bit-equality of
y_lo with bf16_round(y) is the whole check.
"""
import numpy as np
import pytest

from tests import _strict as S
from tests import _strict_norm as N

F32, F64 = np.float32, np.float64
CASES = N.LN_CASES
IDS = [c.id for c in CASES]
BY_ID = {c.id: i for i, c in enumerate(CASES)}


def _ln(i, defect=None, store_mode="rne"):
    c, x, g, b, ref, bound = N.ln_case_data(i)
    y, guard = N.emu_layernorm(x, g, b, N.EPS, c.dout, c.geom, defect=defect, store_mode=store_mode)
    a, bias = N.judge(y, ref, bound, c.dout)
    return c, a, bias, guard


def _fails(i, defect=None, store_mode="rne"):
    c, a, bias, guard = _ln(i, defect, store_mode)
    return not (a["ok"] and bias["ok"] and bool((guard == N.SENTINEL).all()))


# ================================================================================================ the case tables
def test_case_tables_reach_what_they_claim():
    shapes = {c.geom[2:] for c in N.LN_VEC}
    assert shapes == {(1, 16), (1, 32), (1, 64), (2, 64), (3, 64), (4, 64), (6, 64), (8, 64)}
    for c in N.LN_VEC:
        assert c.id.startswith(f"nch{c.nch}_ch{c.geom[2]}w{c.geom[3]}")
    # the grid-stride cases: 2048 blocks of 4 waves; 16485 row groups = 2 * 8192 + 101
    assert N.vec_blocks(8, 65937) == (2048, 16485) and N.vec_blocks(33, 16485) == (2048, 16485)
    assert N.vec_shape(8)[1] == 16 and N.vec_shape(33) == (1, 64)
    assert {c.expect for c in CASES} == {"layernorm", "layernorm_vec", "layernorm_slim"}
    for c in CASES:
        assert N.route(c.C, c.din, c.dout, c.gamma, c.beta, c.stride, c.flags) == c.expect, c.id
    assert [N.pm_nv(C) for _, _, _, C in N.PM_CASES] == [2, 2, 2, 2, 3, 3, 6, 6]
    B, H, W, C = N.PM_GRIDSTRIDE
    assert B * (H // 2) * (W // 2) == 8281 > 8192
    g = {rc: N.mom_geometry(*rc) for rc in N.MOM_CASES + [N.MOM_CAP]}
    assert g[(1, 8)][1] == 256 and g[(200, 24)][2] == 1 and g[(1000, 96)][2] == 4 and g[(37, 1032)][2] == 127
    assert g[(37, 2040)][1] == 1 and g[(37, 2048)][1] == 1 and g[(37, 2048)][3] == 3
    assert g[(1107, 2048)][3] == 70 and g[(23189, 96)][3] == 70 and 48 < 70 < 64 + 16
    assert g[N.MOM_CAP][3] == N.MOM_BLOCKS and -(-N.MOM_CAP[0] // 16) == N.MOM_BLOCKS


def test_bias_cases_are_sized_by_the_reference():
    """Every bf16-output case of M C >= 8192 unit-variance elements has the 4096 reference elements the bias rule asks for."""
    n = 0
    for i, c in enumerate(CASES):
        if c.dout == "bf16" and c.M * c.C >= 8192 and c.kind == "gauss":
            ref = N.ln_case_data(i)[4]
            assert int((np.abs(ref) >= 2.0 ** -6).sum()) >= N.BIAS_MIN_ELEMS, c.id
            n += 1
    assert n >= 20


# ================================================================================================ correct emulations pass
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_layernorm_emulation_passes(i):
    c, a, bias, guard = _ln(i)
    assert a["ok"], a
    assert bias["ok"], bias
    assert (guard == N.SENTINEL).all()
    x, idx = N.rep_rows(c.M, c.C, c.din)
    g, b = N.affine_of(c.C, c.gamma, c.beta)
    ref, bound = N.ln_ref_bound(x, g, b, None, N.EPS, c.dout, k_mean=c.k_mean)
    y, _ = N.emu_layernorm(x, g, b, N.EPS, c.dout, c.geom)
    assert N.judge_rep(y, idx, ref, bound, c.dout) == []


@pytest.mark.parametrize("nch,zd,res,lo", N.ADD_CASES + [N.ADD_GRIDSTRIDE[1:2] + N.ADD_GRIDSTRIDE[2:]])
def test_layernorm_add_emulation_passes(nch, zd, res, lo):
    if nch == N.ADD_GRIDSTRIDE[1]:
        M, C = N.ADD_GRIDSTRIDE[:2]
    else:
        M, C = 37, nch * N.EPC[zd]
    z, r, g, b, ref, bound = N.add_data(M, C, zd, res)
    y, ylo = N.emu_layernorm_add(z, r, g, b, N.EPS, lo, ("vec", N.EPC[zd]) + N.vec_shape(C // N.EPC[zd]))
    a = S.check_bound(y, ref, None, 0, "fp32", bound=bound)
    assert a["ok"], a
    if lo is not None:
        assert S.check_exact(ylo, S.store(y, lo))["ok"]


@pytest.mark.parametrize("out", ["bf16", "fp32"])
@pytest.mark.parametrize("B,H,W,C", N.PM_CASES + [N.PM_GRIDSTRIDE])
def test_patch_merge_ln_emulation_passes(B, H, W, C, out):
    x, g, b = N.pm_data(B, H, W, C)
    ref, bound = N.ln_ref_bound(N.merge_rows(x), g, b, None, N.EPS, out, k_mean=1, k_mul=2, k_add=1)
    a, bias = N.judge(N.emu_patch_merge_ln(x, g, b, N.EPS, out), ref, bound, out)
    assert a["ok"] and bias["ok"], (a, bias)


# ================================================================================================ LayerNorm defects
LN_DEFECT_CASES = {
    "one_pass": ["nch32_ch1w32_M37_fp32_fp32_offset4096"],
    "no_eps": ["nch13_ch1w16_M37_bf16_bf16_const", "nch65_ch2w64_M37_fp32_fp32_const", "nch13_ch1w16_M37_fp32_fp32_sigma0.01"],
    "eps_outside": ["nch13_ch1w16_M37_fp32_fp32_sigma0.01", "generic_C22_M7_fp32_fp32"],
    "c_minus_1": ["nch13_ch1w16_M37_bf16_bf16", "nch512_ch8w64_M37_fp32_fp32", "slim_C768_M5", "generic_C70_M7_bf16_bf16"],
    "dead_chunk": ["nch13_ch1w16_M37_fp32_fp32", "nch24_ch1w32_M37_fp32_fp32", "nch33_ch1w64_M37_fp32_fp32",
                   "nch65_ch2w64_M37_fp32_fp32", "nch129_ch3w64_M37_fp32_fp32", "nch193_ch4w64_M37_fp32_fp32",
                   "nch257_ch6w64_M37_bf16_bf16", "nch385_ch8w64_M37_bf16_fp32"],
    "prev_subrow": ["nch13_ch1w16_M5_bf16_bf16", "nch13_ch1w16_M5_fp32_fp32"],
    "store_clamped": ["nch13_ch1w16_M5_bf16_bf16", "nch24_ch1w32_M37_fp32_bf16"],
    "gb_late": ["nch13_ch1w16_M37_bf16_bf16", "nch65_ch2w64_M37_fp32_fp32", "nch24_ch1w32_M37_bf16_fp32_g_only",
                "nch129_ch3w64_M37_fp32_fp32_b_only"],
}


@pytest.mark.parametrize("defect,case", [(d, c) for d, cs in LN_DEFECT_CASES.items() for c in cs])
def test_layernorm_defect_fails_its_case(defect, case):
    i = BY_ID[case]
    assert not _fails(i), "the correct emulation must pass first"
    assert _fails(i, defect), f"{defect} survives {case}"


def test_full_width_rows_have_no_dead_chunk():
    """The converse: at the full-width rows the dead-chunk switch changes nothing -- the ragged cases are the ones that see it."""
    for case in ("nch16_ch1w16_M37_fp32_fp32", "nch64_ch1w64_M37_fp32_fp32", "nch512_ch8w64_M37_fp32_fp32"):
        c, x, g, b, _, _ = N.ln_case_data(BY_ID[case])
        assert np.array_equal(N.emu_layernorm(x, g, b, N.EPS, c.dout, c.geom)[0],
                              N.emu_layernorm(x, g, b, N.EPS, c.dout, c.geom, defect="dead_chunk")[0])


@pytest.mark.parametrize("case", ["nch13_ch1w16_M5_bf16_bf16", "nch24_ch1w32_M37_fp32_fp32"])
def test_prev_subrow_breaks_row_invariance_and_isolation(case):
    c = CASES[BY_ID[case]]
    x, idx = N.rep_rows(c.M, c.C, c.din)
    g, b = N.affine_of(c.C)
    ref, bound = N.ln_ref_bound(x, g, b, None, N.EPS, c.dout)
    y, _ = N.emu_layernorm(x, g, b, N.EPS, c.dout, c.geom, defect="prev_subrow")
    assert N.judge_rep(y, idx, ref, bound, c.dout) != []


@pytest.mark.parametrize("case", ["nch65_ch2w64_M37_bf16_bf16", "nch129_ch3w64_M37_fp32_bf16", "nch192_ch3w64_M5_fp32_bf16_no_ln_slim",
                                  "generic_C520_M37_bf16_bf16_forced", "nch33_ch1w64_M16485_bf16_bf16_gridstride"])
def test_truncating_store_fails_the_bias(case):
    """Truncation stays inside the per-element bound of most elements; the bias instrument is what sees it.  The M = 5 slim shapes
    have at most 3840 elements: below the rule's count, so the rule does not apply there -- M = 8195 is the slim kernel's bias case."""
    i = BY_ID[case]
    c, a, bias, _ = _ln(i, store_mode="trunc")
    if c.M * c.C >= 8192:
        assert not bias["ok"] and bias["bias"] < -0.3, bias
    else:
        assert bias["n_bias"] == 0
    c2, a2, bias2, _ = _ln(BY_ID["slim_C256_M8195_gridstride"], store_mode="trunc")
    assert not bias2["ok"]


def test_patch_merge_swap_fails():
    for out in ("bf16", "fp32"):
        for B, H, W, C in N.PM_CASES:
            x, g, b = N.pm_data(B, H, W, C)
            ref, bound = N.ln_ref_bound(N.merge_rows(x), g, b, None, N.EPS, out, k_mean=1, k_mul=2, k_add=1)
            a, _ = N.judge(N.emu_patch_merge_ln(x, g, b, N.EPS, out, swap12=True), ref, bound, out)
            assert not a["ok"], (C, out)
    x, g, b = N.pm_data(*N.PM_CASES[3])
    ref, bound = N.ln_ref_bound(N.merge_rows(x), g, b, None, N.EPS, "bf16", k_mean=1, k_mul=2, k_add=1)
    _, bias = N.judge(N.emu_patch_merge_ln(x, g, b, N.EPS, "bf16", store_mode="trunc"), ref, bound, "bf16")
    assert not bias["ok"] and bias["n_bias"] >= N.BIAS_MIN_ELEMS      # 12 rows of 512
    x, g, b = N.pm_data(*N.PM_GRIDSTRIDE)
    ref, bound = N.ln_ref_bound(N.merge_rows(x), g, b, None, N.EPS, "bf16", k_mean=1, k_mul=2, k_add=1)
    _, bias = N.judge(N.emu_patch_merge_ln(x, g, b, N.EPS, "bf16", store_mode="trunc"), ref, bound, "bf16")
    assert not bias["ok"]


# ================================================================================================ moments
MOM = [(r, c, d) for r, c in N.MOM_CASES for d in ("bf16", "fp32")] + [N.MOM_CAP + ("bf16",)]
MOM_IDS = [f"{r}x{c}_{d}" for r, c, d in MOM]


@pytest.mark.parametrize("rows,C,dtype", MOM, ids=MOM_IDS)
def test_moments_emulation_passes_both_instruments(rows, C, dtype):
    x, shift = N.mom_data(rows, C, dtype, "int")
    N.prove_mom_exact(f"{rows}x{C}", x, shift, rows)
    s1, _ = N.mom_ref(x, None, 1)
    d1, _ = N.mom_ref(x, shift, 1)
    d2, _ = N.mom_ref(x, shift, 2)
    assert S.check_exact(N.emu_moments(x, None, "sum"), s1)["ok"]
    assert S.check_exact(N.emu_moments(x, shift, "sq"), d2)["ok"]
    assert S.check_exact(N.emu_moments(x, shift, "both"), np.concatenate([d1, d2]))["ok"]
    if rows * C > 1 << 22:
        return                                   # the cap case: the bound instrument runs at the smaller shapes
    x, shift = N.mom_data(rows, C, dtype, "gauss")
    for mode, sh, p in (("sum", None, 1), ("sq", shift, 2)):
        ref, mag = N.mom_ref(x, sh, p)
        a = S.check_bound(N.emu_moments(x, sh, mode), ref, None, 0, "fp32", bound=N.mom_bound(rows, mag))
        assert a["ok"], (mode, a)


@pytest.mark.parametrize("sigmas", [0.0, 0.3, 3.0])
@pytest.mark.parametrize("rows,C", [(1000, 96), (37, 2048)])
def test_moments2_emulation_passes_at_every_shift(rows, C, sigmas):
    x, shift = N.mom_data(rows, C, "fp32", "gauss", sigmas)
    (r1, m1), (r2, m2) = N.mom_ref(x, shift, 1), N.mom_ref(x, shift, 2)
    a = S.check_bound(N.emu_moments(x, shift, "both"), np.concatenate([r1, r2]), None, 0, "fp32",
                      bound=N.mom_bound(rows, np.concatenate([m1, m2])))
    assert a["ok"], a


@pytest.mark.parametrize("defect,mode", [("tail_skip", "sum"), ("tail_skip", "both"), ("double_count", "sq"), ("double_count", "both"),
                                         ("read_past_G", "sum"), ("read_past_G", "both"), ("square_first", "sq")])
def test_moments_defect_fails_37x2048(defect, mode):
    """37 x 2048: G = 3, every block has 12 or 13 rows -- block 0 runs the unrolled loop three times and the tail once."""
    x, shift = N.mom_data(37, 2048, "bf16", "int")
    sh = None if mode == "sum" else shift
    p = {"sum": [1], "sq": [2], "both": [1, 2]}[mode]
    ref = np.concatenate([N.mom_ref(x, sh, q)[0] for q in p])
    assert S.check_exact(N.emu_moments(x, sh, mode), ref)["ok"]
    got = N.emu_moments(x, sh, mode, defect=defect)
    assert not S.check_exact(got, ref)["ok"], defect
    if defect == "read_past_G":
        assert np.isnan(got).all()


# ================================================================================================ fold kernels
@pytest.mark.parametrize("affine", [True, False], ids=["affine", "no_affine"])
@pytest.mark.parametrize("first_time", [0, 1])
@pytest.mark.parametrize("C", [8, 264])
def test_fold_emulations_pass(C, first_time, affine):
    d = N.fold_data(C)
    w, b = (d["weight"], d["bias"]) if affine else (None, None)
    ref, mag, n_ops = N.bn_mean_ref(d["sum"], d["n"])
    assert S.check_bound(N.emu_bn_mean(d["sum"], d["n"]), ref, mag, 0, "fp32", n_ops=n_ops)["ok"]
    refs = N.fold_ref(d["sqdev"], d["mean"], d["n"], d["run_mean"], d["run_var"], w, b, d["momentum"], d["eps"], first_time)
    got = N.emu_fold(d["sqdev"], d["mean"], d["n"], d["run_mean"], d["run_var"], w, b, d["momentum"], d["eps"], first_time)
    for k, (ref, mag, n_ops) in refs.items():
        a = S.check_bound(got[k], ref, mag, 0, "fp32", n_ops=n_ops)
        assert a["ok"], (k, a)
    if not first_time:
        refs = N.fold1_ref(d["sums"], d["n"], d["run_mean"], d["run_var"], w, b, d["momentum"], d["eps"])
        got = N.emu_fold1(d["sums"], d["n"], d["run_mean"], d["run_var"], w, b, d["momentum"], d["eps"])
        for k, (ref, bound) in refs.items():
            a = S.check_bound(got[k], ref, None, 0, "fp32", bound=bound)
            assert a["ok"], (k, a)


def test_fold1_bound_grows_with_the_offset_of_the_shift():
    """The cancellation term: at |mean - shift| = 3 sigma the variance bound is (1 + 2 * 9) / 1 times the one at the mean, to the
    first term."""
    n, C = 1568.0, 8
    out = []
    for k in (0.0, 3.0):
        d = np.full(C, k)                       # sigma = 1
        sums = np.concatenate([n * d, n * (1.0 + d * d)]).astype(F32)
        _, bound = N.fold1_ref(sums, n, np.zeros(C, F32), np.zeros(C, F32), None, None, 0.0, 1e-5)["run_var"]
        out.append(float(bound[0]))
    assert 5.0 < out[1] / out[0] < 19.0, out


@pytest.mark.parametrize("C", [8, 264])
def test_fold1_constant_channels_and_the_clamp(C):
    sums, _ = N.const_sums(C)
    d = N.fold_data(C)
    for rv0 in (d["run_var"], np.zeros(C, F32)):
        ref = N.fold1_ref(sums, 1568.0, d["run_mean"], rv0, None, None, d["momentum"], d["eps"])
        got = N.emu_fold1(sums, 1568.0, d["run_mean"], rv0, None, None, d["momentum"], d["eps"])
        rv, bound = ref["run_var"]
        assert (got["run_var"] >= 0).all() and np.isfinite(got["run_var"]).all()
        # variance 0 up to the residue of the rounded sums: run_var = momentum * run_var_old within the bound
        target = float(d["momentum"]) * rv0.astype(F64)
        assert (np.abs(got["run_var"] - target) <= bound + np.abs(rv - target)).all()
        assert S.check_bound(got["run_var"], rv, None, 0, "fp32", bound=bound)["ok"]
    # the defect: without fmaxf some channel's fp32 residue is negative, and with run_var = 0 so is the new running variance
    bad = N.emu_fold1(sums, 1568.0, d["run_mean"], np.zeros(C, F32), None, None, d["momentum"], d["eps"], clamp=False)
    assert (bad["run_var"] < 0).any(), "no constant channel leaves a negative residue: the clamp is not exercised"
