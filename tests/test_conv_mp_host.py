"""CPU: the instruments of tests/test_conv_mp_gpu.py see the defects they are there to catch, the preconditions of its exact cases hold,
the restated split arithmetic reaches every regime, the model emulation is far above fp32 noise, and
`filter_value_and_grad(..., conv_dtype=...)` validates its keyword when the decorator is applied (no device needed)."""
import functools

import numpy as np
import pytest

from tests import _conv_mp_ref as R
from tests import _linear_mp_ref as L
from tests import _strict as S

F64 = np.float64
IDS = [g.tag for g in R.SHAPES]


def _as32(a):
    return np.asarray(a, F64).astype(np.float32).astype(F64)


# ================================================================================================ the references
@pytest.mark.parametrize("g", R.SHAPES + [R.SPLIT_SHAPE], ids=IDS + [R.SPLIT_SHAPE.tag])
def test_references_are_the_autograd_convolution(g):
    """With the identity for a rounding the three references are torch's float64 convolution and its autograd gradients."""
    x, w, dy, _ = R.gauss_case(g)
    y = S._conv64(x, w, (g.sh, g.sw), (g.ph, g.pw), (g.dh, g.dw), 1)
    dx, dw = S.conv_bwd64(x, w, dy, g)
    for entry, want in (("fwd", y), ("dgrad", dx), ("wgrad", dw)):
        got, mag = R.product_ref(entry, g, x, w, dy, rnd=R.identity)
        assert got.shape == R.out_shape(entry, g) == want.shape
        assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), entry
        assert (mag >= np.abs(got) - 1e-12).all()


# ================================================================================================ the exact cases see the defects
ROUNDINGS = [("truncate", dict(rnd=L.trunc_bf16)), ("half_away", dict(rnd=L.half_away_bf16)), ("no_rounding", dict(rnd=R.identity)),
             ("rounded_bias", dict(rnd_bias=L.rne_bf16))]
ROUNDING_CASES = [(n, kw, e) for n, kw in ROUNDINGS for e in R.ENTRIES if n != "rounded_bias" or e == "fwd"]


@pytest.mark.parametrize("name,kw,entry", ROUNDING_CASES, ids=[f"{c[0]}-{c[2]}" for c in ROUNDING_CASES])
def test_round_case_sees_defect(name, kw, entry):
    """A kernel with the defect computes, at best, the float64 value of the defective formula rounded to fp32: S.check_exact, the judge
    of the GPU test, must fail on it -- and pass on the reference itself, which is fp32-exact."""
    g = R.ROUND_SHAPES[entry]
    x, w, dy, bias = R.round_case(entry)
    ref, _ = R.product_ref(entry, g, x, w, dy, bias)
    bad, _ = R.product_ref(entry, g, x, w, dy, bias, **kw)
    assert not S.check_exact(_as32(bad), ref)["ok"]
    assert S.check_exact(_as32(ref), ref)["ok"]


def _sees(entry, g, defect):
    x, w, dy, bias = R.int_case(g)
    ref, _ = R.product_ref(entry, g, x, w, dy)
    bad, _ = R.product_ref(entry, g, x, w, dy, defect=defect)
    return not S.check_exact(_as32(bad), ref)["ok"]


def test_int_cases_see_the_geometry_defects():
    s3, s4, s5, s6, s7, s8 = (R.SHAPES[i] for i in (2, 3, 4, 5, 6, 7))
    # a dgrad that takes floor((hi + ph - r dh) / sh) without asking whether the stride divides: every strided shape
    for g in (s3, s5, s6, s7):
        assert _sees("dgrad", g, "dgrad_no_stride_test"), g.tag
    # taps transposed (r and s swapped) on shape 5, R != S: all three entries
    for entry in R.ENTRIES:
        assert _sees(entry, s5, "taps_transposed"), entry
    # dilation ignored on shape 4: all three entries
    for entry in R.ENTRIES:
        assert _sees(entry, s4, "dilation_ignored"), entry
    # a wgrad that drops its last ragged chunk of positions: shape 8 (363 = 11 x 32 + 11), shape 3, and the split shape
    for g in (s8, s3, R.SPLIT_SHAPE):
        assert g.P % R.KSTEP != 0 and _sees("wgrad", g, "wgrad_drops_ragged_chunk"), g.tag


# ================================================================================================ preconditions
@pytest.mark.parametrize("entry", R.ENTRIES)
@pytest.mark.parametrize("g", R.SHAPES + [R.SPLIT_SHAPE], ids=IDS + [R.SPLIT_SHAPE.tag])
def test_int_case_preconditions(g, entry):
    x, w, dy, bias = R.int_case(g)
    for t in (x, w, dy, bias):
        assert np.array_equal(L.rne_bf16(t), t) and np.abs(t).max() <= 2
    for b in ((None, bias) if entry == "fwd" else (None,)):
        ref, mag = R.product_ref(entry, g, x, w, dy, b)
        S.prove_exact(f"{entry}/{g.tag}", ref, mag, R.weights_of(entry, g, x, w, dy), out="fp32")
        assert S.check_exact(_as32(ref), ref)["ok"]


@pytest.mark.parametrize("entry", R.ENTRIES)
def test_round_case_preconditions(entry):
    g = R.ROUND_SHAPES[entry]
    x, w, dy, bias = R.round_case(entry)
    ref, mag = R.product_ref(entry, g, x, w, dy, bias)
    R.prove_round_case(entry, g, ref, mag, x, w, dy, bias)                 # S.prove_exact(..., out="fp32", frac_bits=16) inside


def test_shapes_reach_what_they_are_there_for():
    s = R.SHAPES
    assert [g.P for g in s] == [1, 25, 40, 64, 60, 72, 9, 363, 9] and s[8].Wo == 1
    assert s[7].P > 2 * R.TILE and s[7].P % R.TILE != 0 and s[7].Ho * s[7].Wo < R.TILE          # three row tiles, rows cross images
    assert s[3].C > R.KSTEP and s[3].C % R.KSTEP and s[3].K == R.TILE + 2
    assert s[1].C == 3 and s[5].C % 2 == 1 and s[5].K % 2 == 1
    assert (s[4].R, s[4].S) == (1, 7) and s[4].sh != s[4].sw and s[4].ph != s[4].pw
    assert all(R.kred_of(e, R.ROUND_SHAPES[e]) == 16 for e in R.ENTRIES)


# ================================================================================================ the split arithmetic
def test_wgrad_split_of_the_regime_cases():
    """The split shape wants 3 parts of 288 positions and leaves the last one ragged (240); shape 8 wants one.  The fit2 offer runs two
    parts, fit1 and no offer one."""
    g, sync = R.SPLIT_SHAPE, 4096
    out = g.out_elems * 4
    assert g.P == 816 and R.wgrad_split(g, 8 << 20) == (3, 3, 288) and g.P - 2 * 288 == 240
    assert R.wgrad_split(g, None)[:2] == (3, 1)
    assert R.wgrad_split(g, sync + int(2.5 * out))[:2] == (3, 2)
    assert R.wgrad_split(g, sync + int(1.5 * out))[:2] == (3, 1)
    for offer in (None, 8 << 20, sync + int(2.5 * R.SHAPES[7].out_elems * 4)):
        assert R.wgrad_split(R.SHAPES[7], offer)[:2] == (1, 1)
    big = R.BOUND_SHAPES[-1]
    assert R.wgrad_split(big, 8 << 20)[:2] == (1, 1) and big.P == 392


# ================================================================================================ the model references
def test_resnet_emulation_is_above_fp32_noise():
    """(b) against (a): the effect of rounding every convolution's operands to bf16 on the gradient, relative L2 over all parameters.  It
    has to be far above fp32 noise (1e-4) for the GPU test's ratio to mean anything, and small enough to be a rounding effect."""
    ref = R.resnet_refs()
    names = ref["names"]
    a = np.concatenate([np.asarray(ref["a"][1][n], F64).reshape(-1) for n in names])
    b = np.concatenate([np.asarray(ref["b"][1][n], F64).reshape(-1) for n in names])
    d = float(np.linalg.norm(b - a) / np.linalg.norm(a))
    print(f"resnet18 emulation: rel L2 (b) vs (a) {d:.3e}; loss (a) {ref['a'][0]:.6f} (b) {ref['b'][0]:.6f}")
    assert 1e-4 < d < 0.1
    assert np.isfinite(b).all() and len(names) == len(ref["b"][1])


# ================================================================================================ the keyword
def test_conv_dtype_is_checked_at_decoration():
    import eqxvision_amd as eqv

    def fn(model, x):
        return None
    with pytest.raises(ValueError):
        eqv.filter_value_and_grad(fn, conv_dtype="int8")
    with pytest.raises(ValueError):
        eqv.filter_value_and_grad(conv_dtype="fp16")
    with pytest.raises(ValueError):
        eqv.filter_value_and_grad(matmul_dtype="bf16", conv_dtype="tf32")
    with pytest.raises(ValueError):
        eqv.filter_value_and_grad(matmul_dtype="int8", conv_dtype="bf16")
    with pytest.raises(ValueError):
        functools.partial(eqv.filter_value_and_grad, arg={"w": True}, conv_dtype="int8")(fn)
    assert callable(eqv.filter_value_and_grad(fn, conv_dtype="bf16"))
    assert callable(eqv.filter_value_and_grad(fn, conv_dtype="fp32"))
    assert callable(eqv.filter_value_and_grad(fn, matmul_dtype="bf16", conv_dtype="bf16"))
    spec = {"w": True}
    deco = functools.partial(eqv.filter_value_and_grad, arg=spec, conv_dtype="bf16", matmul_dtype="bf16")
    wrapped = deco(fn)
    assert callable(wrapped) and wrapped.__name__ == "fn"
    inner = eqv.filter_value_and_grad(arg=spec, conv_dtype="bf16")              # the `fn is None` form carries every keyword on
    assert inner.keywords == {"arg": spec, "matmul_dtype": "fp32", "conv_dtype": "bf16"}
    assert callable(inner(fn)) and inner(fn).__name__ == "fn"
