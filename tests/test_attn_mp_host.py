"""CPU proofs for the mixed-precision attention core (tests/_attn_mp_ref.py; the device side is tests/test_attn_mp_gpu.py).

1. The float64 formulas, with r = identity, agree with torch.autograd on softmax(q k^T scale) v in float64, and the lse form of the
   backward equals the kept-probabilities form.
2. Every construction holds (prove_exact_case) and the clean float32 emulation of the kernel passes every instrument at every shape
   of the GPU test.
3. Each seeded defect fails the instrument that is meant to see it.
4. `attn_dtype` is validated when the decorator is applied, is kept by functools.partial, and is independent of the other two.
"""
import functools

import numpy as np
import pytest
import torch

from tests import _attn_mp_ref as R

F64 = np.float64
IDS = [R.shape_id(s) for s in R.SHAPES]


def _ident(a):
    return np.asarray(a, F64)


# ================================================================================================ 1. the formulas
@pytest.mark.parametrize("shape", [(2, 5, 8), (3, 33, 16)], ids=["5x8", "33x16"])
def test_formulas_match_autograd(shape):
    G, n, dh = shape
    rng = np.random.default_rng(3)
    q, k, v, dout = (rng.standard_normal((G, n, dh)) for _ in range(4))
    scale = dh ** -0.5
    tq, tk, tv = (torch.tensor(t, dtype=torch.float64, requires_grad=True) for t in (q, k, v))
    L = tq @ tk.transpose(1, 2) * scale
    out = torch.softmax(L, -1) @ tv
    out.backward(torch.tensor(dout))
    f = R.fwd64(q, k, v, scale, rnd=_ident)
    np.testing.assert_allclose(f["out"], out.detach().numpy(), rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(f["lse"], torch.logsumexp(L, -1).detach().numpy(), rtol=1e-12, atol=1e-13)
    b = R.bwd64(q, k, v, f["out"], dout, f["lse"], scale, rnd=_ident)
    bp = R.bwd64_probs(q, k, v, f["probs"], dout, scale, rnd=_ident)
    for t, ref in (("dq", tq.grad), ("dk", tk.grad), ("dv", tv.grad)):
        np.testing.assert_allclose(b[t], ref.numpy(), rtol=1e-10, atol=1e-12)
        np.testing.assert_allclose(b[t], bp[t], rtol=1e-10, atol=1e-12)             # the lse form == the kept-probabilities form


# ================================================================================================ 2. the clean emulation
@pytest.mark.parametrize("shape", R.SHAPES, ids=IDS)
def test_clean_emulation_passes(shape):
    for kind in ("select", "tie", "flat"):
        if kind == "tie" and not R.has_tie(shape):
            continue
        p = R.exact_case(kind, shape)
        R.prove_exact_case(p)
        got = R.emulate(p)
        assert R.check_exact_fwd(got, p)["ok"], (kind, R.check_exact_fwd(got, p))
        if kind != "flat":
            assert R.check_exact_bwd(got, p)["ok"], (kind, R.check_exact_bwd(got, p))
    c = R.gauss_case(shape)
    got = R.emulate(c, want_probs=True)
    info = R.check_gauss(got, c, probs=got["probs"])
    print(f"attn_mp/emulation/{R.shape_id(shape)}: worst error/bound {R.worst(info)}")
    assert info["ok"], info


# ================================================================================================ 3. the seeded defects
def _exact(kind, shape, which, defect):
    p = R.exact_case(kind, shape)
    got = R.emulate(p, **{defect: True})
    return (R.check_exact_fwd if which == "fwd" else R.check_exact_bwd)(got, p)


def _gauss(shape, defect):
    c = R.gauss_case(shape)
    return R.check_gauss(R.emulate(c, **{defect: True}), c)


SEEN_BY = {
    "drop_last_key": lambda: _gauss((2, 2, 65, 64), "drop_last_key")["out"],
    "unmasked_pad": lambda: _exact("flat", (2, 3, 17, 32), "fwd", "unmasked_pad")["out"],
    "truncate_p": lambda: _gauss((1, 1, 197, 64), "truncate_p")["out_bias"],
    "delta_rounded": lambda: _exact("tie", (2, 2, 65, 64), "bwd", "delta_rounded")["dq"],
    "no_scale_ds": lambda: _exact("tie", (2, 3, 17, 32), "bwd", "no_scale_ds")["dk"],
    "swap_dk_dv": lambda: _exact("select", (2, 3, 17, 32), "bwd", "swap_dk_dv")["dv"],
    "skip_last_query_tile": lambda: _exact("select", (2, 2, 65, 64), "bwd", "skip_last_query_tile")["dv"],
    "lse_no_max": lambda: _exact("select", (1, 1, 5, 32), "fwd", "lse_no_max")["lse"],
}


def test_every_defect_has_an_instrument():
    assert set(SEEN_BY) == set(R.DEFECTS)


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_defect_is_seen(defect):
    info = SEEN_BY[defect]()
    assert not info["ok"], f"{defect} passed its instrument: {info}"


def test_defects_are_seen_by_the_gauss_bound_too():
    """The per-element bound alone sees the gross backward defects at the workload's N."""
    for defect, entry in (("no_scale_ds", "dq"), ("swap_dk_dv", "dk"), ("skip_last_query_tile", "dv")):
        assert not _gauss((2, 2, 65, 64), defect)[entry]["ok"], defect


# ================================================================================================ 4. the keyword
def test_attn_dtype_is_checked_at_decoration():
    import eqxvision_amd as eqv

    def fn(model, x):
        return None
    with pytest.raises(ValueError):
        eqv.filter_value_and_grad(fn, attn_dtype="fp16")
    with pytest.raises(ValueError):
        eqv.filter_value_and_grad(attn_dtype="fp16")
    assert callable(eqv.filter_value_and_grad(fn, attn_dtype="bf16"))
    assert callable(eqv.filter_value_and_grad(fn, attn_dtype="fp32"))
    deco = functools.partial(eqv.filter_value_and_grad, arg={"w": True}, attn_dtype="bf16")
    wrapped = deco(fn)
    assert callable(wrapped) and wrapped.__name__ == "fn"
    inner = eqv.filter_value_and_grad(attn_dtype="bf16", matmul_dtype="bf16")            # the keyword-only call returns a partial ...
    assert inner.keywords["attn_dtype"] == "bf16" and inner.keywords["matmul_dtype"] == "bf16" and inner.keywords["conv_dtype"] == "fp32"
    assert callable(inner(fn))                                                            # ... that still takes the function
    from eqxvision_amd import grad
    assert grad.Tape().attn_dtype == "fp32"
