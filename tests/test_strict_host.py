"""CPU self-test of tests/_strict.py: a numpy emulation of the kernel contract (fp32 accumulation in 16-wide chunks, BatchNorm +
residual + ReLU epilogue, bf16 store) goes through the same checkers the GPU module uses.  The correct emulation passes both
instruments; each of five mutants (truncating store, one dropped BatchNorm shift, ReLU skipped just below zero, a dropped reduction
chunk for one N tile, ...) fails at least one; the generator's precondition asserts fire on an over-range recipe.  This proves that
the checkers can fail."""
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
