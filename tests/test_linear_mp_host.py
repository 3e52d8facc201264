"""CPU: the instruments of tests/test_linear_mp_gpu.py see the defects they are there to catch, the preconditions of its exact cases
hold, and `filter_value_and_grad(..., matmul_dtype=...)` validates its keyword when the decorator is applied (no device needed)."""
import functools

import numpy as np
import pytest
import torch

from tests import _linear_mp_ref as R
from tests import _strict as S

F64 = np.float64


# ================================================================================================ the rounding
def _grid():
    """Around every bf16 value of a few binades, both signs: the value, the exact ties above it (both parities occur along the
    mantissa), the fp32 neighbours of the ties, quarter points; plus zeros, tiny and large magnitudes."""
    hi = np.arange(0x3F00, 0x4080, dtype=np.uint32)                       # bf16 patterns of [0.5, 4)
    hi = np.concatenate([hi, np.arange(0x0080, 0x0090, dtype=np.uint32), np.arange(0x7E00, 0x7E10, dtype=np.uint32)])
    lo = np.array([0x0000, 0x0001, 0x4000, 0x7FFF, 0x8000, 0x8001, 0xC000, 0xFFFF], np.uint32)
    u = ((hi[:, None] << 16) | lo[None, :]).reshape(-1)
    u = np.concatenate([u, u | np.uint32(0x80000000), np.array([0, 0x80000000], np.uint32)])
    return u.view(np.float32)


def test_rne_bf16_is_torch_bfloat16():
    a = _grid()
    got = R.rne_bf16(a)
    want = torch.tensor(a).to(torch.bfloat16).float().numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    u = a.view(np.uint32)
    ties = (u & 0xFFFF) == 0x8000
    par = (u >> 16) & 1
    assert (ties & (par == 0)).any() and (ties & (par == 1)).any() and (ties & (a < 0)).any()
    assert ((u & 0xFFFF) == 0x7FFF).any() and ((u & 0xFFFF) == 0x8001).any()
    # ties go to even: down where the kept mantissa is even, up where it is odd
    assert np.array_equal(got.view(np.uint32)[ties & (par == 0)], u[ties & (par == 0)] & np.uint32(0xFFFF0000))
    assert np.array_equal(got.view(np.uint32)[ties & (par == 1)], (u[ties & (par == 1)] & np.uint32(0xFFFF0000)) + np.uint32(0x10000))
    # and the defective roundings do differ from it on this grid
    assert not np.array_equal(R.trunc_bf16(a), got) and not np.array_equal(R.half_away_bf16(a), got)


# ================================================================================================ the exact cases see the defects
DEFECTS = [("truncate", dict(rnd=R.trunc_bf16)), ("half_away", dict(rnd=R.half_away_bf16)), ("no_rounding", dict(rnd=R.identity)),
           ("rounded_bias", dict(rnd_bias=R.rne_bf16))]


DEFECT_CASES = [(n, kw, e) for n, kw in DEFECTS for e in R.ENTRIES if n != "rounded_bias" or e == "fwd"]      # the bias is the forward's


@pytest.mark.parametrize("name,kw,entry", DEFECT_CASES, ids=[f"{c[0]}-{c[2]}" for c in DEFECT_CASES])
def test_round_case_sees_defect(name, kw, entry):
    """A kernel with the defect computes, at best, the float64 value of the defective formula rounded to fp32 (every such value of this
    case is fp32-exact or rounds once): the judge of the GPU test (S.check_exact) must fail on it."""
    x, w, g, bias = R.round_case(entry)
    ref, _ = R.product_ref(entry, x, w, g, bias)
    bad, _ = R.product_ref(entry, x, w, g, bias, **kw)
    bad = bad.astype(np.float32).astype(F64)
    assert not S.check_exact(bad, ref)["ok"]
    assert S.check_exact(ref.astype(np.float32).astype(F64), ref)["ok"]          # the reference itself is fp32-exact


def test_int_case_sees_a_dropped_tile_and_a_swap():
    """The integer cases: a result with one reduction element left out, or with the operands' orientation swapped, is not equal."""
    M, N, K = 130, 129, 65
    x, w, g, bias = R.int_case(M, N, K)
    ref, _ = R.product_ref("fwd", x, w, g, bias)
    short, _ = R.product_ref("fwd", x[:, :-1], w[:, :-1], g, bias)
    assert not S.check_exact(short, ref)["ok"]
    refd, _ = R.product_ref("dgrad", x, w, g)
    sq = R.int_case(64, 64, 64)
    a, _ = R.product_ref("dgrad", sq[0], sq[1], sq[2])
    b, _ = R.product_ref("dgrad", sq[0], sq[1].T.copy(), sq[2])
    assert not S.check_exact(b, a)["ok"] and refd.shape == (M, K)


# ================================================================================================ preconditions, all shapes
@pytest.mark.parametrize("entry", R.ENTRIES)
@pytest.mark.parametrize("shape", R.SHAPES + [(1030, 70, 40), (18145, 70, 40)], ids=R.shape_id)
def test_int_case_preconditions(shape, entry):
    M, N, K = shape
    x, w, g, bias = R.int_case(M, N, K)
    for t in (x, w, g, bias):
        assert np.array_equal(R.rne_bf16(t), t) and np.abs(t).max() <= 2
    for b in ((None, bias) if entry == "fwd" else (None,)):
        ref, mag = R.product_ref(entry, x, w, g, b)
        S.prove_exact(f"{entry}/{shape}", ref, mag, list(R._operands(entry, x, w, g)), out="fp32")
        assert float((ref == 0).mean()) < 0.9


@pytest.mark.parametrize("entry", R.ENTRIES)
def test_round_case_preconditions(entry):
    M, N, K = R.round_shape(entry)
    assert R.kred_of(entry, M, N, K) <= 16 and sorted(set((M, N, K)) - {16}) == [33, 130]
    x, w, g, bias = R.round_case(entry)
    ref, mag = R.product_ref(entry, x, w, g, bias)
    R.prove_round_case(entry, ref, mag, x, w, g, bias)                     # S.prove_exact(..., out="fp32", frac_bits=16) inside
    assert float((ref == 0).mean()) < 0.9


def test_wgrad_split_of_the_regime_cases():
    """M = 1030 wants 4 parts; 18145 wants 64 parts of 288 rows and leaves the last part ONE row; the fit2 offer runs two parts, fit1 none."""
    N, K = 70, 40
    sync, out = 4096, N * K * 4
    assert R.wgrad_split(1030, N, K, 8 << 20)[:2] == (4, 4)
    want, parts, chunk = R.wgrad_split(18145, N, K, 8 << 20)
    assert (want, parts, chunk) == (64, 64, 288) and (parts - 1) * chunk + 1 == 18145
    for M in (1030, 18145):
        assert R.wgrad_split(M, N, K, None)[1] == 1
        assert R.wgrad_split(M, N, K, sync + int(2.5 * out))[1] == 2
        assert R.wgrad_split(M, N, K, sync + int(1.5 * out))[1] == 1
    assert R.wgrad_split(788, 192, 768, 8 << 20)[1] > 1 and R.wgrad_split(257, 96, 40, 8 << 20)[1] == 1


def _old_linear_split(M, N, K, offer=None):
    """The formula _linear_mp_ref.wgrad_split had before it was shared with _conv_mp_ref, verbatim."""
    TILE, KSTEP = 128, 32
    tiles = -(-N // TILE) * -(-K // TILE)
    steps = -(-M // KSTEP)
    want = 1 if tiles >= 1024 else -(-1024 // tiles)
    want = max(1, min(want, steps // 8, 64))
    split = want
    if split > 1:
        fit = 0 if offer is None else max(0, offer - 4096) // (N * K * 4)
        split = 1 if fit < 2 else min(split, fit)
    chunk = -(-steps // split) * KSTEP
    return want, -(-M // chunk), chunk


def _old_conv_split(g, offer=None):
    """The formula _conv_mp_ref.wgrad_split had, verbatim."""
    TILE, KSTEP = 128, 32
    tiles = -(-g.K // TILE) * g.R * g.S * -(-g.C // TILE)
    steps = -(-g.P // KSTEP)
    want = 1 if tiles >= 1024 else -(-1024 // tiles)
    want = max(1, min(want, steps // 8, 64))
    split = want
    if split > 1:
        fit = 0 if offer is None else max(0, offer - 4096) // (g.out_elems * 4)
        split = 1 if fit < 2 else min(split, fit)
    chunk = -(-steps // split) * KSTEP
    return want, -(-g.P // chunk), chunk


def test_shared_wgrad_split_is_both_old_formulas():
    """The one rule (R.wgrad_split_rule, behind R.wgrad_split and _conv_mp_ref.wgrad_split) against the two formulas it replaced, exactly,
    over 1 / 2 / 9 / 1023 / 1024 tiles, reductions around the 8-step and the part boundaries, and offers around one and two parts."""
    import types

    from tests import _conv_mp_ref as CR
    T = 128
    linear = {1: (1, 1), 2: (T + 1, 1), 9: (3 * T, 3 * T), 1023: (33 * T, 31 * T), 1024: (32 * T, 32 * T)}        # tiles: (N, K)
    conv = {1: (1, 1, 1, 1), 2: (1, 2, 1, 1), 9: (1, 3, 3, 1), 1023: (31 * T, 3, 11, 1), 1024: (32 * T, 4, 8, 1)}  # tiles: (K, R, S, C)
    for tiles in (1, 2, 9, 1023, 1024):
        N, K = linear[tiles]
        ck, cr, cs, cc = conv[tiles]
        assert -(-N // T) * -(-K // T) == tiles and -(-ck // T) * cr * cs * -(-cc // T) == tiles
        for red in (1, 255, 256, 257, 1030, 18145):
            g = types.SimpleNamespace(K=ck, R=cr, S=cs, C=cc, P=red, out_elems=ck * cr * cs * cc)
            for out, old, new in ((N * K, lambda o: _old_linear_split(red, N, K, o), lambda o: R.wgrad_split(red, N, K, o)),
                                  (g.out_elems, lambda o: _old_conv_split(g, o), lambda o: CR.wgrad_split(g, o))):
                for offer in (None, 4096, 4096 + out * 4, 4096 + 2 * out * 4, 4096 + 2 * out * 4 - 1, 4096 + 100 * out * 4):
                    assert new(offer) == old(offer) == R.wgrad_split_rule(tiles, red, out, offer), (tiles, red, out, offer)


# ================================================================================================ the model references
def test_vit_emulation_is_above_fp32_noise():
    """(b) against (a): the effect of rounding every Linear's operands to bf16 on the gradient, relative L2 over all parameters.  It has
    to be far above fp32 noise (1e-4) for the GPU test's ratio to mean anything."""
    ref = R.vit_refs()
    names = ref["names"]
    a = np.concatenate([np.asarray(ref["a"][1][n], F64).reshape(-1) for n in names])
    b = np.concatenate([np.asarray(ref["b"][1][n], F64).reshape(-1) for n in names])
    d = float(np.linalg.norm(b - a) / np.linalg.norm(a))
    print(f"vit emulation: rel L2 (b) vs (a) {d:.3e}; loss (a) {ref['a'][0]:.6f} (b) {ref['b'][0]:.6f}")
    assert d > 1e-4 and d < 0.1
    # the head is un-rounded: with the same features its gradient formula is the float64 one -- the patch leaves `fc` alone
    assert np.isfinite(b).all() and len(names) == len(ref["b"][1])


# ================================================================================================ the keyword
def test_matmul_dtype_is_checked_at_decoration():
    import eqxvision_amd as eqv

    def fn(model, x):
        return None
    with pytest.raises(ValueError):
        eqv.filter_value_and_grad(fn, matmul_dtype="int8")
    with pytest.raises(ValueError):
        eqv.filter_value_and_grad(matmul_dtype="int8")
    assert callable(eqv.filter_value_and_grad(fn, matmul_dtype="bf16"))
    assert callable(eqv.filter_value_and_grad(fn, matmul_dtype="fp32"))
    spec = {"w": True}
    deco = functools.partial(eqv.filter_value_and_grad, arg=spec, matmul_dtype="bf16")
    wrapped = deco(fn)
    assert callable(wrapped) and wrapped.__name__ == "fn"
    assert callable(eqv.filter_value_and_grad(matmul_dtype="bf16")(fn))
