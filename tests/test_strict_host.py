"""CPU self-test of tests/_strict.py: a numpy emulation of the kernel contract (fp32 accumulation in 16-wide chunks, BatchNorm +
residual + ReLU epilogue, bf16 store) goes through the same checkers the GPU module uses.  The correct emulation passes both
instruments; each of five mutants (truncating store, one dropped BatchNorm shift, ReLU skipped just below zero, a dropped reduction
chunk for one N tile, ...) fails at least one; the generator's precondition asserts fire on an over-range recipe.  This proves that
the checkers can fail.

The second half does the same for the memory-bound kernels (tests/test_strict_mem_gpu.py): ten mutants of the emulations at the GPU
module's shapes, the three that the old global criterion lets through, and the rounding-bias limit as a condition on the inputs."""
import numpy as np
import pytest

from tests import _strict as S

SHAPES = [(600, 64, 64), (600, 1152, 128), (300, 4608, 64)]          # M x K_red x N
IDS = [f"{m}x{k}x{n}" for m, k, n in SHAPES]
_CACHE = {}


def _gauss(M, K, N):
    key = ("g", M, K, N)
    if key not in _CACHE:
        rng = S.rng_of(1000 + K)
        x = S.bf(rng.standard_normal((M, K)))
        w = S.bf(rng.standard_normal((N, K)) / np.sqrt(K))
        sc = S.gauss_scale(rng, N)
        sh = (0.1 * rng.standard_normal(N)).astype(np.float32)
        res = S.bf(rng.standard_normal((M, N)))
        ref, mag = S.gemm_ref(x, w, sc, sh, res, 1)
        _CACHE[key] = (x, w, sc, sh, res, ref, mag)
    return _CACHE[key]


def _ints(M, K, N, nnz=32, xlim=2):
    key = ("i", M, K, N, nnz, xlim)
    if key not in _CACHE:
        rng = S.rng_of(2000 + K)
        x = S.int_tensor(rng, (M, K), xlim)
        w = S.pm1_rows(rng, N, K, nnz)
        sc = S.int_scale(rng, N)
        sh = S.int_tensor(rng, (N,), 8)
        res = S.int_tensor(rng, (M, N), 16)
        ref, mag = S.gemm_ref(x, w, sc, sh, res, 1)
        _CACHE[key] = (x, w, sc, sh, res, ref, mag)
    return _CACHE[key]


def _nnz(K, N):
    return max(32, -(-K // N))          # enough entries per row to cover the reduction


def _instrument2(got, ref, mag, K):
    a = S.check_bound(got, ref, mag, K, "bf16")
    b = S.check_bias(got, ref) if K <= S.BIAS_MAX_KRED else {"ok": True, "bias": float("nan"), "n_bias": 0}
    return a, b


@pytest.mark.parametrize("M,K,N", SHAPES, ids=IDS)
def test_correct_emulation_passes_both_instruments(M, K, N):
    x, w, sc, sh, res, ref, mag = _ints(M, K, N, _nnz(K, N), 1 if K > 1152 else 2)
    S.prove_exact("host", ref, mag, [w], stored=[x, w, sc, sh, res])
    e = S.check_exact(S.emulate(x, w, sc, sh, res, 1), ref)
    assert e["ok"], e
    x, w, sc, sh, res, ref, mag = _gauss(M, K, N)
    a, b = _instrument2(S.emulate(x, w, sc, sh, res, 1), ref, mag, K)
    print(f"correct {M}x{K}x{N}: worst |got-ref|/bound {a['worst']:.3f}, bias {b['bias']:+.4f} over {b['n_bias']}, n {a['n']}")
    assert a["ok"] and a["worst"] <= 1.0, a
    assert b["ok"], b


@pytest.mark.parametrize("M,K,N", SHAPES[:2], ids=IDS[:2])
def test_mutant_truncating_store(M, K, N):
    x, w, sc, sh, res, ref, mag = _gauss(M, K, N)
    a, b = _instrument2(S.emulate(x, w, sc, sh, res, 1, store="trunc"), ref, mag, K)
    print(f"trunc {M}x{K}x{N}: {a['nviol']} of {a['n']} over the bound, worst {a['worst']:.2f}, bias {b['bias']:+.3f}")
    # the accumulation term of the bound grows with K_red: the per-element bound is sure to see truncation at K_red = 64, the bias
    # wherever it applies (K_red <= 1152).  At K_red = 4608 neither instrument sees it (test_truncation_blind_spot_at_long_k).
    if K == 64:
        assert not a["ok"] and a["nviol"] > a["n"] // 10
    assert not b["ok"] and -0.55 < b["bias"] < -0.45


def test_truncation_blind_spot_at_long_k():
    """the documented limit of instrument 2: at K_red = 4608 the accumulation term exceeds a bf16 ulp for most elements and the bias
    does not apply, so a truncating store mostly hides -- far fewer violations than at K_red = 64; the GPU module therefore keeps a
    short-K case for every kernel family."""
    M, K, N = SHAPES[2]
    x, w, sc, sh, res, ref, mag = _gauss(M, K, N)
    a = S.check_bound(S.emulate(x, w, sc, sh, res, 1, store="trunc"), ref, mag, K, "bf16")
    e_pre = (K + 4) * 2.0 ** -23 * mag
    assert np.median(e_pre / (2 * S.half_ulp_out(np.abs(ref) + e_pre, "bf16"))) > 0.5          # why: e_pre alone is over half an ulp
    assert a["nviol"] < a["n"] // 100


@pytest.mark.parametrize("M,K,N", SHAPES, ids=IDS)
def test_mutant_dropped_shift(M, K, N):
    x, w, sc, sh, res, ref, mag = _gauss(M, K, N)
    k = int(np.argmax(np.abs(sh) > 0.02))
    a, _ = _instrument2(S.emulate(x, w, sc, sh, res, 1, drop_shift_channel=k), ref, mag, K)
    print(f"shift {M}x{K}x{N}: channel {k} (shift {sh[k]:+.3f}), worst {a['worst']:.1f}, channels {a.get('bad_channels')}")
    assert not a["ok"] and a["bad_channels"] == [k]
    x, w, sc, sh, res, ref, mag = _ints(M, K, N, _nnz(K, N), 1 if K > 1152 else 2)
    k = int(np.argmax(sh != 0))
    e = S.check_exact(S.emulate(x, w, sc, sh, res, 1, drop_shift_channel=k), ref)
    assert not e["ok"] and e["bad_channels"] == [k]


@pytest.mark.parametrize("M,K,N", SHAPES, ids=IDS)
def test_mutant_relu_skipped_below_zero(M, K, N):
    x, w, sc, sh, res, ref, mag = _gauss(M, K, N)
    a, _ = _instrument2(S.emulate(x, w, sc, sh, res, 1, relu_skip_above=-0.03), ref, mag, K)
    print(f"relu {M}x{K}x{N}: {a['nviol']} over the bound, worst {a['worst']:.0f}")
    assert not a["ok"] and a["worst"] > (10 if K <= S.BIAS_MAX_KRED else 1)


@pytest.mark.parametrize("M,K,N", SHAPES, ids=IDS)
def test_mutant_dropped_chunk_fails_exact(M, K, N):
    x, w, sc, sh, res, ref, mag = _ints(M, K, N, _nnz(K, N), 1 if K > 1152 else 2)
    got = S.emulate(x, w, sc, sh, res, 1, drop_chunk=(K // 16 - 1, 32, 64))          # the last 16-wide k-step of N tile 32 .. 63
    e = S.check_exact(got, ref)
    print(f"chunk {M}x{K}x{N}: {e.get('nbad')} wrong, channels {e.get('bad_channels')}")
    assert not e["ok"] and all(32 <= c < 64 for c in e["bad_channels"])


def test_mutant_wrong_residual_element_fails_exact():
    """a fifth kind of defect the exact instrument names: the residual read from the neighbouring row for one channel."""
    M, K, N = SHAPES[0]
    x, w, sc, sh, res, ref, mag = _ints(M, K, N)
    r2 = res.copy()
    r2[:, 7] = np.roll(res[:, 7], 1)
    e = S.check_exact(S.emulate(x, w, sc, sh, r2, 1), ref)
    assert not e["ok"] and e["bad_channels"] == [7]


def test_generator_covers_and_stays_in_range():
    """the ranges of the issue: nnz = 32 at K_red = 1152 -- full coverage, magnitudes within bf16's exact integers."""
    x, w, sc, sh, res, ref, mag = _ints(600, 1152, 128)
    assert (np.abs(w).sum(1) == 32).all() and set(np.unique(w)) == {-1.0, 0.0, 1.0}
    assert (w != 0).any(0).all()
    assert set(np.unique(np.abs(sc))) <= {1.0, 2.0} and (sc < 0).any() and (sc > 0).any()
    assert np.abs(sh).max() <= 8 and np.abs(res).max() <= 16
    assert mag.max() <= 2 * 32 * 2 + 8 + 16 <= S.BF16_INT_MAX
    assert (ref == 0).mean() < 0.9
    assert np.array_equal(S.bf(ref), ref.astype(np.float32))


def test_preconditions_fire_on_over_range_recipes():
    rng = S.rng_of(5)
    M, K, N = 64, 256, 32
    w = S.pm1_rows(rng, N, K, 64)
    sc, sh = S.int_scale(rng, N), S.int_tensor(rng, (N,), 8)
    x = S.int_tensor(rng, (M, K), 4)                                   # 64 * 4 * 2 + 8 > 256
    ref, mag = S.gemm_ref(x, w, sc, sh, None, 0)
    with pytest.raises(AssertionError, match="not exact in bf16"):
        S.prove_exact("over", ref, mag, [w], stored=[x, w])
    x = S.int_tensor(rng, (M, K), 1)
    ref, mag = S.gemm_ref(x, w, sc, sh, None, 0)
    S.prove_exact("fine", ref, mag, [w], stored=[x, w])
    with pytest.raises(AssertionError, match="not exact in bf16"):
        S.prove_exact("big operand", ref, mag, [w], stored=[x * 300])
    with pytest.raises(AssertionError, match="not integer-valued"):
        S.prove_exact("fraction", ref + 0.5, mag, [w])
    w0 = w.copy()
    w0[:, 5] = 0
    with pytest.raises(AssertionError, match="reduction indices unused"):
        S.prove_exact("hole", ref, mag, [w0])
    w0 = w.copy()
    w0[3] = 0
    with pytest.raises(AssertionError, match="all-zero output channels"):
        S.prove_exact("dead row", ref, mag, [w0])
    with pytest.raises(AssertionError, match="are zero"):
        S.prove_exact("blank", np.zeros_like(ref), mag, [w])
    with pytest.raises(AssertionError, match="2\\^24"):
        S.prove_exact("acc", ref, mag * 2.0 ** 20, [w], out="fp32")
    with pytest.raises(AssertionError, match="cannot cover"):
        S.pm1_rows(rng, 4, 1024, 32)


def test_half_ulp_and_bias_definitions():
    assert S.half_ulp_out(1.0, "bf16") == 2.0 ** -8 and S.half_ulp_out(1.99, "bf16") == 2.0 ** -8
    assert S.half_ulp_out(2.0, "bf16") == 2.0 ** -7 and S.half_ulp_out(0.0, "bf16") == 0.0
    assert S.half_ulp_out(1.0, "fp32") == 2.0 ** -24
    ref = np.linspace(0.02, 7.0, 9000)
    b, n = S.rounding_bias(S.bf16_truncate(ref), ref)
    assert n > 8000
    assert -0.55 < b < -0.45
    b, _ = S.rounding_bias(S.bf(ref), ref)
    assert abs(b) < 0.02


# ================================================================================================ memory-bound kernels
# The emulations of tests/_strict.py at the shapes of tests/test_strict_mem_gpu.py: the unmutated emulation passes the instrument the
# GPU case uses, each mutant fails it.
def _bound(got, ref, mag, n_ops, out, bound=None):
    return S.check_bound(got, ref, mag, 0, out, n_ops=n_ops, bound=bound)


def _act_case(act="hard_swish", n=40008, dtype="bf16"):
    x = S.act_input(S.rng_of(40), n, dtype)
    ref = S.act64(x, act)
    return x, ref, S.act_n_ops(x, act)


@pytest.mark.parametrize("act", ["hard_swish", "silu"])
def test_mem_mutant_truncating_store(act):
    x, ref, n_ops = _act_case(act)
    good = S.emu_eltwise(x, act, "bf16")
    a, b = _bound(good, ref, np.abs(ref), n_ops, "bf16"), S.check_bias(good, ref)
    assert a["ok"] and b["ok"], (a, b)
    bad = S.emu_eltwise(x, act, "bf16", store_mode="trunc")
    a, b = _bound(bad, ref, np.abs(ref), n_ops, "bf16"), S.check_bias(bad, ref)
    print(f"mem trunc {act}: {a['nviol']} of {a['n']} over the bound, bias {b['bias']:+.3f}")
    # hard_swish returns its bf16 input unchanged above 3 (no rounding at all there), which dilutes truncation's -0.5
    assert not a["ok"] and a["nviol"] > a["n"] // 10
    assert not b["ok"] and -0.55 < b["bias"] < (-0.2 if act == "hard_swish" else -0.45)


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_mem_mutant_shift_from_channel_plus_8(dtype):
    x, sc, sh, _ = S.affine_data(50, 24, dtype)
    ref, mag = S.affine_ref(x, sc, sh, None, "relu")
    for vec8 in (True, False):
        assert _bound(S.emu_channel_affine(x, sc, sh, None, "relu", dtype, vec8=vec8), ref, mag, 2, dtype)["ok"]
    a = _bound(S.emu_channel_affine(x, sc, sh, None, "relu", dtype, shift_from=8), ref, mag, 2, dtype)
    assert not a["ok"] and a["n_bad_channels"] == 24


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("rows,C", [(50, 24), (33, 264)])
def test_mem_mutant_residual_dropped_in_last_vector(rows, C, dtype):
    x, sc, sh, r = S.affine_data(rows, C, dtype, res=True)
    ref, mag = S.affine_ref(x, sc, sh, r, "none")
    assert _bound(S.emu_channel_affine(x, sc, sh, r, "none", dtype), ref, mag, 3, dtype)["ok"]
    a = _bound(S.emu_channel_affine(x, sc, sh, r, "none", dtype, drop_res_last_vec=True), ref, mag, 3, dtype)
    assert not a["ok"] and 1 <= a["nviol"] <= 8 and all(c >= C - 8 for c in a["bad_channels"])


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_mem_mutant_relu_skipped_just_below_zero(dtype):
    x, sc, sh, r = S.affine_data(33, 264, dtype, res=True)
    ref, mag = S.affine_ref(x, sc, sh, r, "relu")
    assert _bound(S.emu_channel_affine(x, sc, sh, r, "relu", dtype), ref, mag, 3, dtype)["ok"]
    a = _bound(S.emu_channel_affine(x, sc, sh, r, "relu", dtype, relu_skip_above=-2.0 ** -7), ref, mag, 3, dtype)
    assert not a["ok"] and a["nviol"] >= 1
    rng = S.rng_of(41)
    p, q = (S.q_of(dtype)(rng.standard_normal(40008)) for _ in range(2))
    ref = S.act64(p.astype(np.float64) + q, "relu")
    mag = np.abs(p).astype(np.float64) + np.abs(q)
    assert _bound(S.emu_add(p, q, "relu", dtype), ref, mag, 1, dtype)["ok"]
    assert not _bound(S.emu_add(p, q, "relu", dtype, relu_skip_above=-2.0 ** -7), ref, mag, 1, dtype)["ok"]


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("k,s,p", [(3, 2, 1), (3, 1, 1)])
def test_mem_mutant_maxpool_padding_read_as_zero(k, s, p, dtype):
    x = S.q_of(dtype)(-2.0 - np.abs(S.wide_data(S.rng_of(21), (2, 9, 11, 13), dtype)))
    ref = S.maxpool64(x, k, s, p)
    assert S.check_exact(S.emu_maxpool(x, k, s, p), ref)["ok"]
    e = S.check_exact(S.emu_maxpool(x, k, s, p, pad_value=0.0), ref)
    assert not e["ok"] and e["nbad"] > 0
    # with Gaussian data of both signs the same mutant is seen too, at the border windows whose taps are all negative
    x = S.wide_data(S.rng_of(21), (2, 9, 11, 13), dtype)
    assert not S.check_exact(S.emu_maxpool(x, k, s, p, pad_value=0.0), S.maxpool64(x, k, s, p))["ok"]


@pytest.mark.parametrize("dout", ["bf16", "fp32"])
def test_mem_mutant_adaptive_window_neighbour_count(dout):
    x = S.bf(S.rng_of(44).standard_normal((2, 7, 5, 13)))
    ref, mag, win = S.adaptive_ref(x, 3, 2)
    assert _bound(S.emu_adaptive_avgpool(x, 3, 2, dout), ref, mag, win + 2, dout)["ok"]
    assert not _bound(S.emu_adaptive_avgpool(x, 3, 2, dout, neighbour_count=True), ref, mag, win + 2, dout)["ok"]


def test_mem_mutant_last_grid_stride_trip_not_written():
    """The two grid-stride cases: 2^21 vectors of 8 per trip (eltwise_x8), 2^20 elements per trip (scalar add)."""
    rng = S.rng_of(29)
    n = 8 * (2 ** 21 + 257)
    x = rng.integers(-64, 65, n, dtype=np.int8)
    ref = np.maximum(x, 0)
    assert np.array_equal(S.emu_eltwise(x, "relu", "bf16"), ref)
    bad = S.emu_eltwise(x, "relu", "bf16", drop_last_trip=8 * 2 ** 21)
    assert not np.array_equal(bad, ref) and int((bad != ref).sum()) == 8 * 257 - int((ref[-8 * 257:] == S.SENTINEL).sum())
    n = 2 ** 20 + 257
    a, b = (rng.integers(-64, 65, n).astype(np.float32) for _ in range(2))
    ref = np.maximum(a + b, 0)
    assert S.check_exact(S.emu_add(a, b, "relu", "bf16"), ref)["ok"]
    e = S.check_exact(S.emu_add(a, b, "relu", "bf16", drop_last_trip=2 ** 20), ref)
    assert not e["ok"] and e["nbad"] == 257 and e["first"][0][0] == (2 ** 20,)
    # a size below one trip has no second trip to lose: the small cases cannot see this defect
    assert S.check_exact(S.emu_add(a[:100003], b[:100003], "relu", "bf16", drop_last_trip=2 ** 20)[:0], ref[:0])["ok"]


@pytest.mark.parametrize("shape,lane", [((2, 25, 25, 40), 7), ((3, 7, 7, 264), 31)])
def test_mem_mutant_avgpool_lane_lost(shape, lane):
    cpb, pl, idle, blocks = S.wide_geometry(shape[3])
    x = S.bf(S.rng_of(44).standard_normal(shape))
    ref, mag, win = S.adaptive_ref(x, 1, 1)
    flat = x.reshape(shape[0], -1, shape[3])
    for dout in ("bf16", "fp32"):
        good = S.emu_global_avgpool(flat, dout, pl)[:, None, None, :]
        assert _bound(good, ref, mag, win + 2, dout)["ok"]
        bad = S.emu_global_avgpool(flat, dout, pl, lost_lane=lane)[:, None, None, :]
        assert not _bound(bad, ref, mag, win + 2, dout)["ok"]
    xi = S.int_tensor(S.rng_of(30), (2, 16, 16, 64), 8)
    ri, _, _ = S.adaptive_ref(xi, 1, 1)
    fi = xi.reshape(2, 256, 64)
    assert S.check_exact(S.emu_global_avgpool(fi, "fp32", 32)[:, None, None, :], ri)["ok"]
    assert not S.check_exact(S.emu_global_avgpool(fi, "fp32", 32, lost_lane=5)[:, None, None, :], ri)["ok"]


@pytest.mark.parametrize("dout", ["bf16", "fp32"])
def test_mem_mutant_resize_unclamped_tap(dout):
    x = (S.rng_of(32).integers(-8, 9, (2, 7, 5, 3)) * 16).astype(np.float32)
    ref, _ = S.resize_ref(x, 14, 10)
    assert S.check_exact(S.emu_resize(x, 14, 10, dout), ref)["ok"]
    assert not S.check_exact(S.emu_resize(x, 14, 10, dout, clamp=False), ref)["ok"]
    for (h, w, H, W) in ((7, 5, 17, 13), (9, 9, 33, 33), (9, 9, 33, 36)):
        x = S.bf(S.rng_of(33).standard_normal((2, h, w, 3)))
        ref, M = S.resize_ref(x, H, W)
        bound = S.resize_bound(ref, M, h, w, dout)
        a = _bound(S.emu_resize(x, H, W, dout), ref, None, None, dout, bound=bound)
        assert a["ok"], a
        assert not _bound(S.emu_resize(x, H, W, dout, clamp=False), ref, None, None, dout, bound=bound)["ok"]


def test_mem_resize_taps_exact_at_power_of_two_ratios():
    from oracle import np_ops as O
    for n_in, n_out in ((7, 14), (5, 10), (8, 32)):
        assert np.array_equal(S.tap_matrix32(n_in, n_out), O._resize_weights(n_in, n_out))
    assert not np.array_equal(S.tap_matrix32(7, 17), O._resize_weights(7, 17))          # ragged: the float32 weights are rounded


def test_mem_mutant_cast_by_truncation():
    from oracle import np_ops as O
    x = S.wide_data(S.rng_of(22), (100003,), "fp32")
    ref = O.bf16_round(x)
    assert S.check_exact(S.emu_cast(x, "bf16"), ref)["ok"]
    e = S.check_exact(S.emu_cast(x, "bf16", trunc=True), ref)
    assert not e["ok"] and e["nbad"] > 40000


def test_mem_other_emulations_pass_their_instruments():
    """The emulations no mutant above goes through: channel scale, the plain average pool, the backward kernels."""
    for dtype in ("bf16", "fp32"):
        x, s = S.scale_data(72, dtype)
        ref = x.astype(np.float64) * s.astype(np.float64)[:, None, :]
        assert _bound(S.emu_channel_scale(x, s, dtype), ref, np.abs(ref), 1, dtype)["ok"]
        assert not _bound(S.emu_channel_scale(x, s, dtype, store_mode="trunc"), ref, np.abs(ref), 1, dtype)["ok"] or dtype == "fp32"
        x = S.q_of(dtype)(S.rng_of(45).standard_normal((2, 7, 9, 13)))
        ref, mag = S.avgpool2d_ref(x, 3, 2)
        assert _bound(S.emu_avgpool2d(x, 3, 2, dtype), ref, mag, 11, dtype)["ok"]
    rng = S.rng_of(46)
    g, x = (rng.standard_normal((3, 50, 72)).astype(np.float32) for _ in range(2))
    ref, mag = (g.astype(np.float64) * x).sum(1), (np.abs(g).astype(np.float64) * np.abs(x)).sum(1)
    assert _bound(S.emu_channel_scale_bwd(g, x), ref, mag, 52, "fp32")["ok"]
    assert not _bound(S.emu_channel_scale_bwd(g[:, :49], x[:, :49]), ref, mag, 52, "fp32")["ok"]          # one position lost


def test_mem_old_criterion_blind_spots():
    """The gap being closed: three mutants pass `_cases._cmp` at the old tolerances (1e-2 for bf16) and fail the new instruments.
    The dropped residual passes the old criterion where the residual is below 1 % of the tensor's largest value (a residual
    stream 2^-8 of the branch here); at unit scale the old criterion does see it."""
    from tests._cases import TOL_BF16, _cmp
    x = S.bf(S.rng_of(0).uniform(-8, 8, 100003))                  # eltwise_act_case's own data
    ref = S.act64(x, "hard_swish")
    bad = S.emu_eltwise(x, "hard_swish", "bf16", store_mode="trunc")
    assert _cmp(bad, ref, TOL_BF16)["ok"]
    assert not _bound(bad, ref, np.abs(ref), 4, "bf16")["ok"] and not S.check_bias(bad, ref)["ok"]
    xa, sc, sh, r = S.affine_data(33, 264, "bf16", res=True)
    ref, mag = S.affine_ref(xa, sc, sh, r, "relu")
    bad = S.emu_channel_affine(xa, sc, sh, r, "relu", "bf16", relu_skip_above=-2.0 ** -7)
    assert _cmp(bad, ref, TOL_BF16)["ok"] and not _bound(bad, ref, mag, 3, "bf16")["ok"]
    ref, mag = S.affine_ref(xa, sc, sh, r, "none")
    bad = S.emu_channel_affine(xa, sc, sh, r, "none", "bf16", drop_res_last_vec=True)
    assert not _cmp(bad, ref, TOL_BF16)["ok"] and not _bound(bad, ref, mag, 3, "bf16")["ok"]          # unit-scale residual: both see it
    small = S.bf(r * 2.0 ** -8)
    ref, mag = S.affine_ref(xa, sc, sh, small, "none")
    bad = S.emu_channel_affine(xa, sc, sh, small, "none", "bf16", drop_res_last_vec=True)
    assert _cmp(bad, ref, TOL_BF16)["ok"] and not _bound(bad, ref, mag, 3, "bf16")["ok"]
    assert _bound(S.emu_channel_affine(xa, sc, sh, small, "none", "bf16"), ref, mag, 3, "bf16")["ok"]


def _bias_cases():
    """(tag, emulated bf16 output, reference) of every bound case of test_strict_mem_gpu.py with a bf16 output."""
    for act in ("relu", "gelu_tanh", "hard_swish", "hard_sigmoid", "sigmoid", "silu"):
        for n in (40008, 40003):
            x, ref, _ = _act_case(act, n)
            yield f"eltwise/{act}/{n}", S.emu_eltwise(x, act, "bf16"), ref
    for act in ("none", "relu"):
        for n in (40008, 40003):
            rng = S.rng_of(41)
            a, b = (S.bf(rng.standard_normal(n)) for _ in range(2))
            yield f"add/{act}/{n}", S.emu_add(a, b, act, "bf16"), S.act64(a.astype(np.float64) + b, act)
    for C in (72, 13):
        x, s = S.scale_data(C, "bf16")
        yield f"channel_scale/C{C}", S.emu_channel_scale(x, s, "bf16"), x.astype(np.float64) * s.astype(np.float64)[:, None, :]
    for act in ("none", "relu"):
        x, sc, sh, _ = S.affine_data(50, 24, "bf16")
        yield f"channel_affine/{act}", S.emu_channel_affine(x, sc, sh, None, act, "bf16"), S.affine_ref(x, sc, sh, None, act)[0]
        for rows, C in ((50, 24), (33, 264)):
            x, sc, sh, r = S.affine_data(rows, C, "bf16", res=True)
            yield f"channel_affine_res/{rows}x{C}/{act}", S.emu_channel_affine(x, sc, sh, r, act, "bf16"), S.affine_ref(x, sc, sh, r, act)[0]
    for shape in ((2, 25, 25, 40), (3, 7, 7, 264)):
        x = S.bf(S.rng_of(44).standard_normal(shape))
        yield f"adaptive_avgpool/C{shape[3]}", S.emu_global_avgpool(x.reshape(shape[0], -1, shape[3]), "bf16", S.wide_geometry(shape[3])[1]), \
            S.adaptive_ref(x, 1, 1)[0][:, 0, 0]
    for (h, w, H, W) in ((7, 5, 17, 13), (9, 9, 33, 33)):
        x = S.bf(S.rng_of(33).standard_normal((2, h, w, 3)))
        yield f"resize/{h}x{w}->{H}x{W}", S.emu_resize(x, H, W, "bf16"), S.resize_ref(x, H, W)[0]


def test_mem_bias_limit_holds_for_rne_on_every_eligible_case():
    """The rounding-bias limit is a condition on the inputs: with at least 4096 eligible elements (|ref| >= 2^-6) the RNE emulation
    alone must stay within |b| <= 0.05.  Which cases are eligible is pinned here."""
    eligible = []
    for tag, got, ref in _bias_cases():
        n = int((np.abs(ref) >= 2.0 ** -6).sum())
        if n < S.BIAS_MIN_ELEMS:
            continue
        b = S.check_bias(got, ref)
        print(f"bias {tag}: {b['bias']:+.4f} over {b['n_bias']}")
        assert b["ok"], (tag, b)
        eligible.append(tag)
    acts = ("relu", "gelu_tanh", "hard_swish", "hard_sigmoid", "sigmoid", "silu")
    assert eligible == [f"eltwise/{a}/{n}" for a in acts for n in (40008, 40003)] + \
        [f"add/{a}/{n}" for a in ("none", "relu") for n in (40008, 40003)] + \
        ["channel_scale/C72", "channel_affine_res/33x264/none", "channel_affine_res/33x264/relu", "resize/9x9->33x33"], eligible


def test_ops_bound_definition():
    ref, mag = np.array([1.0, -3.0, 0.0]), np.array([2.0, 3.0, 0.0])
    e = 5 * 2.0 ** -23 * mag
    assert np.array_equal(S.ops_bound(ref, mag, 5, "bf16"), e + S.half_ulp_out(np.abs(ref) + e, "bf16"))
    assert S.ops_bound(1.0, 1.0, 0, "fp32") == 2.0 ** -24
    assert np.array_equal(S.ops_bound(ref, mag, 60, "bf16"), S.elem_bound(ref, mag, 56, "bf16"))          # the same 2^-23 per operation
    a = S.check_bound(ref + 1e-3, ref, mag, 0, "fp32", n_ops=1)
    assert not a["ok"] and a["nviol"] == 3
    assert S.check_bound(ref, ref, mag, 0, "fp32", bound=np.zeros(3))["ok"]
