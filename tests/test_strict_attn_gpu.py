"""`-m gpu`: the softmax attention kernels against the instruments of tests/_strict_attn.py (select / tie / flat / mask: logits
chosen so that the softmax is exactly representable, each construction proved on the CPU first; Gaussian operands: a derived
per-element bound and the rounding bias).  Kernels are called through the C ABI into sentinel-filled destinations with a guard
behind them; every case asserts the kernel that served it and prints "exact" or its worst |got - ref| / bound (`pytest -s`).

Measured on the MI355X (worst |got - ref| / bound over the cases of a kernel; no constant was tuned, the bound is the derivation
in tests/_strict_attn.py):
    kernel                         select / tie        flat    mask    Gaussian out   bias (ulp)          probs
    mha_mfma_dh64 [_hm]            exact, probs 0.000  0.731   -       0.620          -0.0032 / 67509     0.012
    mha_mfma_dh32 [_hm]            exact, probs 0.000  0.767   -       0.726          -0.0042 / 8367      0.024
    mha_mfma_dh64 [_hm] dropout    exact, probs 0.000  -       -       -              -                   -
    mha_generic bf16               exact, probs 0.000  0.712   -       0.983          -                   0.064
    mha_generic fp32               0.000               0.019   -       0.009          -                   0.056
    mha_f32_lds                    0.000               0.020   -       0.015          -                   0.062
    swin_attn_mfma                 exact               0.893   0.830   0.834          +0.0095 / 31260     -
    swin_attn_mfma_dropout         exact               -       -       -              -                   -
    swin_attn_generic bf16         exact               0.865   0.830   0.967          -                   -
    swin_attn_f32_lds              0.000               0.026   0.023   0.009          -                   -
    swin_attn_mfma_cos             exact               0.828   0.830   -              -                   -
The bias column is the largest |mean signed error| in output ulps over the kernel's Gaussian cases, every one of which has at
least 4096 eligible elements (asserted; the N = 17 and N = 33 cases run at B = 8 and B = 4 for it).  Limit 0.05; the float32
emulation with a truncated P gives -0.20 .. -0.42.  No kernel defect was found.
"""
import numpy as np
import pytest
import torch

from eqxvision_amd import random as jr
from oracle import np_ops as O
from tests import _strict as ST
from tests import _strict_attn as A
from tests._slices import GUARD, SENTINEL, _dest, _p, _stream

pytestmark = pytest.mark.gpu
TD = {"bf16": torch.bfloat16, "fp32": torch.float32}
_ids = lambda shapes: ["x".join(str(v) for v in s) for s in shapes]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from eqxvision_amd import _lib
    _lib.load()
    _lib.check_device_status()
    yield
    _lib.check_device_status()


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(TD[dtype]).cuda()


def _back(buf, shape):
    """The destination's payload as float64 numpy; sentinel guard intact, nothing non-finite."""
    host = buf.float().cpu()
    n = int(np.prod(shape))
    assert host.numel() == n + GUARD and bool((host[n:] == SENTINEL).all()), "guard overwritten"
    got = host[:n].reshape(shape).double().numpy()
    assert np.isfinite(got).all(), "non-finite output"
    return got


def _keys(B, seed=3):
    ks = jr.split(jr.PRNGKey(seed), B)
    return [ks[b] for b in range(B)], torch.from_numpy(np.asarray(ks, np.uint32).view(np.int32).reshape(B, 2).copy()).cuda()


def _run_mha(p, shape, dtype="bf16", probs=True, head_major=False, generic=False, keys=None, keep=1.0):
    """Returns (out groups (B H, N, dh), probs groups (B H, N, N) or None, kernel)."""
    from eqxvision_amd import _lib
    B, N, H, dh = shape
    qd = _dev(A.mha_pack(p["q"], p["k"], p["v"], B, H, head_major), dtype)
    y = _dest(B * N, H * dh, TD[dtype])
    pr = _dest(B * H * N, N, torch.float32) if probs else None
    dt = _lib.BF16 if dtype == "bf16" else _lib.F32
    _lib.set_flag("force_generic", 1 if generic else 0)
    try:
        if keys is not None:
            _lib.call("mv_mha_dropout_fwd", _p(qd), 1 if head_major else 0, _p(y), _p(pr), _p(keys), float(keep), B, N, H, dh,
                      float(p["scale"]), dt, _stream())
        else:
            _lib.call("mv_mha_heads_fwd" if head_major else "mv_mha_fwd", _p(qd), _p(y), _p(pr), B, N, H, dh, float(p["scale"]), dt, _stream())
        kern = _lib.last_kernel()
    finally:
        _lib.set_flag("force_generic", 0)
    torch.cuda.synchronize()
    out = A.mha_groups(_back(y, (B, N, H * dh)), H)
    return out, (_back(pr, (B * H, N, N)) if probs else None), kern


def _run_swin(p, shape, dtype="bf16", generic=False, keys=None, keep=1.0, cos=False):
    from eqxvision_amd import _lib
    B, Hf, C, heads, ws, shift = shape
    qd = _dev(A.swin_pack(p["q"], p["k"], p["v"], B, Hf, heads, ws, shift), dtype)
    Hf, Wf = A.hw(Hf)
    bd = torch.from_numpy(p["bias"]).cuda()
    y = _dest(B * Hf * Wf, C, TD[dtype])
    dt = _lib.BF16 if dtype == "bf16" else _lib.F32
    _lib.set_flag("force_generic", 1 if generic else 0)
    try:
        if cos:
            rn = torch.ones(B, 2, ws * ws, C, dtype=torch.float32, device="cuda")
            mul = torch.tensor([20.0, 100.0][:heads], dtype=torch.float32, device="cuda")
            _lib.call("mv_swin_window_attn_cos_fwd", _p(qd), _p(rn), _p(mul), _p(bd), _p(y), None, 1.0, B, Hf, Wf, C, heads, ws, ws,
                      shift, shift, dt, _stream())
        elif keys is not None:
            _lib.call("mv_swin_window_attn_dropout_fwd", _p(qd), _p(bd), _p(y), _p(keys), float(keep), B, Hf, Wf, C, heads, ws, ws,
                      shift, shift, dt, _stream())
        else:
            _lib.call("mv_swin_window_attn_fwd", _p(qd), _p(bd), _p(y), B, Hf, Wf, C, heads, ws, ws, shift, shift, dt, _stream())
        kern = _lib.last_kernel()
    finally:
        _lib.set_flag("force_generic", 0)
    torch.cuda.synchronize()
    return A.swin_groups(_back(y, (B, Hf, Wf, C)), heads, ws, shift), kern


def _say(tag, *infos):
    txt = " ".join(f"{n} {i['worst'] if isinstance(i['worst'], str) else format(i['worst'], '.3f')}" for n, i in infos)
    print(f"{tag}: {txt}")
    for n, i in infos:
        assert i["ok"], (tag, n, i)


def _mha_suite(shape, kern, dtype="bf16", probs=True, head_major=False, generic=False, kinds=("select", "tie", "flat", "gauss"), mfma=True):
    base = shape
    for kind in kinds:
        shape = A.gauss_shape(base) if kind == "gauss" and mfma else base          # enough elements for the rounding bias
        p = A.mha_problem(kind, shape, 3 if kind != "gauss" else 4, dtype)
        if kind != "gauss":
            A.prove(p)
        out, pr, k = _run_mha(p, shape, dtype, probs, head_major, generic)
        assert k == kern, (k, kern)
        if kind == "gauss":
            infos = [("out", A.check_gauss(out, p, out=dtype, mfma=mfma))]
            if mfma:
                infos.append(("bias", {"ok": True, "worst": f"{infos[0][1]['bias']:+.4f}/{infos[0][1]['n_bias']}"}))
            if probs:
                infos.append(("probs", A.check_gauss_probs(pr, p)))
        else:
            infos = [("out", A.check_exactish(kind, out, p, dtype))]
            if probs:
                infos.append(("probs", A.check_probs(kind, pr, p)))
        _say(f"{kern} {shape} {dtype} {kind}{' +probs' if probs else ''}", *infos)


# ------------------------------------------------------------------------------------------------ mv_mha_fwd / mv_mha_heads_fwd
@pytest.mark.parametrize("probs", [True, False], ids=["probs", "noprobs"])
@pytest.mark.parametrize("shape", A.MHA_SHAPES, ids=_ids(A.MHA_SHAPES))
def test_mha_mfma(shape, probs):
    _mha_suite(shape, f"mha_mfma_dh{shape[3]}", probs=probs)


@pytest.mark.parametrize("shape", A.MHA_HM_SHAPES, ids=_ids(A.MHA_HM_SHAPES))
def test_mha_heads(shape):
    _mha_suite(shape, f"mha_mfma_dh{shape[3]}_hm", head_major=True, kinds=("select", "tie", "flat"))


@pytest.mark.parametrize("case", A.MHA_DROP_SHAPES, ids=_ids(A.MHA_DROP_SHAPES))
def test_mha_dropout(case):
    """p = 0.5: 1 / keep = 2 is exact.  select: 2 v[pi(i)] where the draw keeps the key, 0 where it drops it; tie: the kept keys' sum."""
    shape, hm = case[:4], case[4]
    B, N, H, dh = shape
    klist, kd = _keys(B)
    keep = np.stack([np.asarray(O.jax_bernoulli(np.asarray(k, np.uint32), np.float32(0.5), (1, H, N, N)))[0] for k in klist])
    km = keep.reshape(B * H, N, N).astype(np.float64) * 2.0
    assert 0.45 < keep.mean() < 0.55
    for kind in ("select", "tie"):
        p = A.mha_problem(kind, shape, 3)
        A.prove(p)
        out, pr, k = _run_mha(p, shape, head_major=hm, keys=kd, keep=0.5)
        assert k == f"mha_mfma_dh{dh}" + ("_hm" if hm else "")
        i1 = ST.check_exact(out, A.expect_dropped(p, km))
        i1["worst"] = "exact" if i1["ok"] else "NOT exact"
        _say(f"{k} dropout {shape} {kind}", ("out", i1), ("probs", A.check_probs(kind, pr, p, km)))


@pytest.mark.parametrize("case", A.MHA_OTHER, ids=_ids(A.MHA_OTHER))
def test_mha_generic_paths(case):
    shape, dtype, generic, kern = case[:4], case[4], case[5], case[6]
    _mha_suite(shape, kern, dtype=dtype, generic=generic, mfma=False)


# ------------------------------------------------------------------------------------------------ Swin
def _swin_suite(shape, kern, dtype="bf16", generic=False, cos=False, tie_codes=True, gauss=True, mfma=True, gauss_B=None):
    """gauss_B: the batch of the Gaussian case where the shape's own gives the rounding-bias rule too few elements (as A.gauss_shape)."""
    B, Hf, C, heads, ws, shift = shape
    cases = [("select", True), ("tie", True), ("flat", True)]
    cases.append(("select", False))
    if tie_codes:
        cases.append(("tie", False))
    if cos:
        cases = [("select", True), ("flat", True)]
    if any(A.eff_shift(L, ws, shift) for L in A.hw(Hf)):
        cases.append(("mask", True))
    if gauss:
        cases.append(("gauss", True))
    for kind, by_bias in cases:
        if kind == "gauss" and gauss_B:
            shape = (gauss_B,) + tuple(shape[1:])
        p, extra = A.swin_problem(kind, shape, 5 if kind != "gauss" else 6, by_bias, dtype=dtype)
        if kind != "gauss":
            A.prove(p, extra)
        out, k = _run_swin(p, shape, dtype, generic, cos=cos)
        assert k == kern, (k, kern)
        if kind == "gauss":
            info = A.check_gauss(out, p, extra, out=dtype, mfma=mfma)
            extra_txt = f" bias {info['bias']:+.4f}/{info['n_bias']}" if mfma else ""
        else:
            info, extra_txt = A.check_exactish(kind, out, p, dtype), ""
        _say(f"{kern} {shape} {dtype} {kind} {'bias' if by_bias else 'codes'}{extra_txt}", ("out", info))


@pytest.mark.parametrize("shape", A.SWIN_SHAPES, ids=_ids(A.SWIN_SHAPES))
def test_swin_mfma(shape):
    _swin_suite(shape, "swin_attn_mfma")


@pytest.mark.parametrize("case", A.SWIN_OTHER, ids=_ids(A.SWIN_OTHER))
def test_swin_generic_paths(case):
    """The tie by codes needs a power-of-two scale here (dh = 16): these kernels scale q by dh^-0.5 BEFORE the dot product, so at
    dh = 32 two equal integer dot products need not round alike; there the tie comes from the bias (form (a)) only."""
    shape, dtype, generic, kern = case[:6], case[6], case[7], case[8]
    _swin_suite(shape, kern, dtype=dtype, generic=generic, tie_codes=(shape[2] // shape[3] == 16), mfma=False)


@pytest.mark.parametrize("shape", A.SWIN_WRAP_SHAPES, ids=_ids(A.SWIN_WRAP_SHAPES))
def test_swin_one_axis_wrap(shape):
    """One window along the axis it covers (that shift is dropped), wrap at shift = ws - 1 along the other: the un-rolled row of
    swin_geom.h is one conditional subtract, exact because y + shift < 2 Hf.  The matrix-core kernel and both fallback kernels.
    B = 1 gives 1024 outputs; the Gaussian case of the matrix-core kernel runs the same map at B = 8 (8192 outputs), because the
    rounding-bias rule needs 4096 eligible elements."""
    _swin_suite(shape, "swin_attn_mfma", gauss_B=8)
    _swin_suite(shape, "swin_attn_generic", generic=True, tie_codes=False, mfma=False)
    _swin_suite(shape, "swin_attn_f32_lds", dtype="fp32", tie_codes=False, mfma=False)


def test_swin_dropout():
    shape = A.SWIN_SHAPES[0]
    B, Hf, C, heads, ws, shift = shape
    n, nW = ws * ws, (Hf // ws) ** 2
    klist, kd = _keys(B)
    keep = np.stack([np.asarray(jr.bernoulli(k, 0.5, (nW, heads, n, n))) for k in klist])
    km = keep.reshape(B * nW * heads, n, n).astype(np.float64) * 2.0
    p, extra = A.swin_problem("select", shape, 5, True)
    A.prove(p, extra)
    out, k = _run_swin(p, shape, keys=kd, keep=0.5)
    assert k == "swin_attn_mfma_dropout"
    info = ST.check_exact(out, A.expect_dropped(p, km))
    info["worst"] = "exact" if info["ok"] else "NOT exact"
    _say(f"{k} {shape} select bias", ("out", info))


@pytest.mark.parametrize("shape", A.COS_SHAPES, ids=_ids(A.COS_SHAPES))
def test_swin_cos(shape):
    """rnorm is an operand: all ones with q = k = 0; the logits are the bias and the mask."""
    _swin_suite(shape, "swin_attn_mfma_cos", cos=True, gauss=False)
