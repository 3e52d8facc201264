"""`-m gpu`: Swin Transformer V2 on the MI355X -- mv_swin_qk_rnorm_fwd, mv_swin_window_attn_cos_fwd and mv_layernorm_add_fwd
against float64 on the same operands (sentinel-filled destinations with a guard behind them, NaN in the value third where it must
not be read), a V2 block and a V2 patch merging through `ops` with the switch "no_swin_v2_fused" off and on, and whole models
against the restatement in tests/_swin_v2_ref.py.  Margins are printed (`pytest -s`).

Conditioning: where a stage has ONE window per image, q / norm(q, axis=0) is sign(q) and the logits are
discontinuous in q.  Such stages are compared in fp32 mode only, behind a guard computed from the restatement alone; with four or
more windows per image ordinary parity applies."""
import math
import warnings

import numpy as np
import pytest
import torch

import eqxvision_amd as eqv
from eqxvision_amd import random as jr
from tests import _strict as ST
from tests import _swin_v2_ref as R
from tests._slices import GUARD, SENTINEL, _dest, _p, _stream

pytestmark = pytest.mark.gpu

FP32_TOL = 1e-3
# (B, Hf, Wf, C, window, shift): one window; shifted 2 x 2 windows; six windows and 12 channel groups; a 4 x 8 window with an uneven
# shift; a 7 x 7 window (49 tokens: padding lanes in the 64-token tile)
SHAPES = ((2, 8, 8, 64, (8, 8), (0, 0)), (1, 16, 16, 64, (8, 8), (4, 4)), (3, 16, 24, 96, (8, 8), (4, 4)),
          (1, 8, 16, 64, (4, 8), (2, 4)), (1, 14, 14, 64, (7, 7), (3, 3)))


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from eqxvision_amd import _lib
    _lib.load()
    _lib.check_device_status()
    yield
    _lib.check_device_status()


def _windows(x, window, shift):
    """x (B, H, W, C) float64 -> (B, nW, n, C)."""
    return torch.stack([R.partition(x[b], list(window), list(shift)) for b in range(x.shape[0])])


def _qkv(B, Hf, Wf, C, dtype, seed, nan_v):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, Hf, Wf, 3 * C, generator=g).to(dtype)
    if nan_v:
        x[..., 2 * C:] = float("nan")
    return x


# ------------------------------------------------------------------------------------------------ 1. mv_swin_qk_rnorm_fwd
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("shape", SHAPES, ids=[f"{s[0]}x{s[1]}x{s[2]}x{s[3]}w{s[4][0]}x{s[4][1]}s{s[5][0]}" for s in SHAPES])
def test_qk_rnorm(shape, dtype):
    """Relative error per element <= (nW + 8) 2^-24: fp32 accumulation of nW squares (one rounding per square, one per add) plus the
    square root and the reciprocal.  The value third is NaN: reading it would poison nothing here, but a NaN in the output would
    show a wrong channel offset; the guard shows a write past the end."""
    from eqxvision_amd import _lib
    B, Hf, Wf, C, win, sh = shape
    n = win[0] * win[1]
    x = _qkv(B, Hf, Wf, C, dtype, 11, True)
    out = _dest(B * 2 * n, C, torch.float32)
    xd = x.cuda()
    _lib.call("mv_swin_qk_rnorm_fwd", _p(xd), _p(out), B, Hf, Wf, C, win[0], win[1], sh[0], sh[1],
              _lib.BF16 if dtype == torch.bfloat16 else _lib.F32, _stream())
    torch.cuda.synchronize()
    host = out.cpu()
    got, guard = host[:B * 2 * n * C].reshape(B, 2, n, C).double(), host[B * 2 * n * C:]
    assert bool((guard == SENTINEL).all()) and guard.numel() == GUARD
    xw = _windows(x.double()[..., :2 * C], win, sh)                          # (B, nW, n, 2C)
    nW = xw.shape[1]
    ref = 1.0 / torch.sqrt((xw * xw).sum(1))                                 # (B, n, 2C)
    ref = torch.stack([ref[..., :C], ref[..., C:]], dim=1)
    assert bool(torch.isfinite(got).all())
    rel = float(((got - ref).abs() / ref).max())
    bound = (nW + 8) * 2.0 ** -24
    print(f"qk_rnorm {shape} {dtype}: nW={nW} rel {rel:.3e} bound {bound:.3e} margin {bound / max(rel, 1e-30):.1f}x")
    assert rel <= bound


def test_qk_rnorm_refuses_partial_windows(built_lib):
    rc = built_lib.mv_swin_qk_rnorm_fwd(1, 1, 1, 12, 16, 64, 8, 8, 0, 0, 1, None)
    assert rc == -2 and b"multiple of the window" in built_lib.mv_last_error()


# ------------------------------------------------------------------------------------------------ 2. mv_swin_window_attn_cos_fwd
LS = (math.log(20.0), math.log(100.0) - 0.05, math.log(100.0) + 0.7)          # below the clamp, within 0.1 of it, above it


def _cos_case(shape, dtype, seed=5):
    B, Hf, Wf, C, win, sh = shape
    heads, n = C // 32, win[0] * win[1]
    x = _qkv(B, Hf, Wf, C, dtype, seed, False)
    xw = _windows(x.double()[..., :2 * C], win, sh)
    rn = (1.0 / torch.sqrt((xw * xw).sum(1))).to(torch.float32)               # (B, n, 2C), made on the host in fp32
    rn = torch.stack([rn[..., :C], rn[..., C:]], dim=1).contiguous()          # (B, 2, n, C)
    ls = torch.tensor([LS[h % 3] for h in range(heads)], dtype=torch.float32)
    mul = torch.exp(torch.clamp(ls, max=math.log(100.0)))
    g = torch.Generator().manual_seed(seed + 1)
    bias = (16 * torch.sigmoid(torch.randn(heads, n, n, generator=g))).to(torch.float32)
    return x, rn, mul, bias


def _cos_ref(x, rn, mul, bias, shape, attn_mask=None):
    """float64 on the same operands; q_hat = T(fp32(q) * rnorm) bit-identically.  Returns (out, sum_j p_j |v_j|, max_j |logit terms|)."""
    B, Hf, Wf, C, win, sh = shape
    heads, n, dh = C // 32, win[0] * win[1], 32
    outs, mags, smag = [], [], []
    for b in range(B):
        xw = R.partition(x[b].float(), list(win), list(sh))                   # (nW, n, 3C), storage values
        nW = xw.shape[0]
        qh = (xw[..., :C] * rn[b, 0]).to(x.dtype).double()
        kh = (xw[..., C:2 * C] * rn[b, 1]).to(x.dtype).double()
        v = xw[..., 2 * C:].double()
        sp = lambda t: t.reshape(nW, n, heads, dh).permute(0, 2, 1, 3)
        qh, kh, v = sp(qh), sp(kh), sp(v)
        m = mul.double().reshape(heads, 1, 1)
        a = qh @ kh.transpose(-2, -1) * m + bias.double()
        am = qh.abs() @ kh.abs().transpose(-2, -1) * m + bias.double().abs()
        mk = R.shift_mask(Hf, Wf, list(win), list(sh))
        if mk is not None:
            a = a + mk[:, None]
            am = am + mk[:, None].abs()
        p = torch.softmax(a, dim=-1)
        if attn_mask is not None:
            p = p * attn_mask[b]
        o = (p @ v).permute(0, 2, 1, 3).reshape(nW, n, C)
        om = (p @ v.abs()).permute(0, 2, 1, 3).reshape(nW, n, C)
        sm = am.max(-1, keepdim=True).values.expand(nW, heads, n, dh).permute(0, 2, 1, 3).reshape(nW, n, C)
        outs.append(R.reverse(o, Hf, Wf, list(win), list(sh)))
        mags.append(R.reverse(om, Hf, Wf, list(win), list(sh)))
        smag.append(R.reverse(sm, Hf, Wf, list(win), list(sh)))
    return torch.stack(outs), torch.stack(mags), torch.stack(smag)


def _launch_cos(x, rn, mul, bias, shape, keys=None, keep=1.0):
    from eqxvision_amd import _lib
    B, Hf, Wf, C, win, sh = shape
    out = _dest(B * Hf * Wf, C, x.dtype)
    xd, rd, md, bd = x.cuda(), rn.cuda(), mul.cuda(), bias.cuda()
    _lib.call("mv_swin_window_attn_cos_fwd", _p(xd), _p(rd), _p(md), _p(bd), _p(out), _p(keys), float(keep), B, Hf, Wf, C, C // 32,
              win[0], win[1], sh[0], sh[1], _lib.BF16 if x.dtype == torch.bfloat16 else _lib.F32, _stream())
    kern = _lib.last_kernel()
    torch.cuda.synchronize()
    host = out.float().cpu()
    guard = host[B * Hf * Wf * C:]
    assert bool((guard == SENTINEL).all()), "guard overwritten"
    return host[:B * Hf * Wf * C].reshape(B, Hf, Wf, C).double(), kern


@pytest.mark.parametrize("shape", SHAPES, ids=[f"{s[0]}x{s[1]}x{s[2]}x{s[3]}w{s[4][0]}x{s[4][1]}s{s[5][0]}" for s in SHAPES])
def test_window_attn_cos_bf16(shape):
    """MFMA path.  Bound per element 2^-7 max|v|: twice the sum of the P rounding and the output rounding (2 (2^-9 + 2^-9) of a convex
    combination of v)."""
    x, rn, mul, bias = _cos_case(shape, torch.bfloat16)
    got, kern = _launch_cos(x, rn, mul, bias, shape)
    assert kern == "swin_attn_mfma_cos"
    ref, _, _ = _cos_ref(x, rn, mul, bias, shape)
    B, Hf, Wf, C, win, sh = shape
    if (Hf // win[0]) * (Wf // win[1]) == 1:                                   # one window: q_hat is exactly +-1
        for b in range(B):
            qh = (x[b, :, :, :C].float() * R.reverse(rn[b, 0], Hf, Wf, list(win), [0, 0])).to(torch.bfloat16).float()
            assert bool((qh.abs() == 1).all())
    assert bool(torch.isfinite(got).all())
    err = float((got - ref).abs().max())
    bound = 2.0 ** -7 * float(x[..., 2 * C:].float().abs().max())
    print(f"attn_cos bf16 {shape}: err {err:.3e} bound {bound:.3e} margin {bound / max(err, 1e-30):.1f}x")
    assert err <= bound


@pytest.mark.parametrize("shape", SHAPES, ids=[f"{s[0]}x{s[1]}x{s[2]}x{s[3]}w{s[4][0]}x{s[4][1]}s{s[5][0]}" for s in SHAPES])
def test_window_attn_cos_fp32(shape):
    """The one-wave-per-query kernel at ops_bound.  A logit is dh fused multiply-adds, the product with logit_mul, the bias and the
    mask: (dh + 3) roundings of S = max_j (sum |q_hat||k_hat| mul + |bias| + |mask|); an absolute error e of a logit is a relative
    error e of its exponential, in the numerator and in the denominator: 2 (dh + 3) S operations.  Then __expf (4), the n-term sum of
    the denominator and of P . V (2 n), the division and q_hat / k_hat's own products (4): n_ops = 2 (dh + 3) S + 2 n + 8, relative to
    sum_j p_j |v_j|."""
    x, rn, mul, bias = _cos_case(shape, torch.float32)
    got, kern = _launch_cos(x, rn, mul, bias, shape)
    assert kern == "swin_attn_generic_cos"
    ref, mag, smag = _cos_ref(x, rn, mul, bias, shape)
    n = shape[4][0] * shape[4][1]
    info = ST.check_bound(got.numpy(), ref.numpy(), mag.numpy(), 0, "fp32", n_ops=(2 * 35 * smag + 2 * n + 8).numpy())
    print(f"attn_cos fp32 {shape}: worst {info['worst']:.3f} of the bound")
    assert info["ok"], info


def test_window_attn_cos_dropout():
    """The reference's attention dropout (swin.py:227): masks from eqv.random on the reference's shape (nW, heads, n, n)."""
    shape = (1, 16, 16, 64, (8, 8), (4, 4))
    p = 0.25
    x, rn, mul, bias = _cos_case(shape, torch.bfloat16, seed=9)
    key = jr.PRNGKey(3)
    keep = jr.bernoulli(key, 1.0 - p, (4, 2, 64, 64))
    mask = torch.from_numpy(np.asarray(keep, np.float64) / (1.0 - p))[None]
    keys = torch.from_numpy(np.asarray(key, np.uint32).view(np.int32).reshape(1, 2).copy()).cuda()
    got, kern = _launch_cos(x, rn, mul, bias, shape, keys=keys, keep=1.0 - p)
    assert kern == "swin_attn_mfma_cos_dropout"
    ref, _, _ = _cos_ref(x, rn, mul, bias, shape, attn_mask=mask)
    err = float((got - ref).abs().max())
    bound = 2.0 ** -7 * float(x[..., 128:].float().abs().max())
    print(f"attn_cos dropout: err {err:.3e} bound {bound:.3e}")
    assert err <= bound


# ------------------------------------------------------------------------------------------------ 3. mv_layernorm_add_fwd
@pytest.mark.parametrize("C", [96, 128, 192, 768, 1024])
@pytest.mark.parametrize("M", [1, 5, 4096])
def test_layernorm_add(M, C):
    """y within ops_bound, y_lo bitwise the round-to-nearest-even of y.  A lane holds at most 16 values of a row: 16 + 6 (the
    cross-lane tree) roundings for each of the two sums, the subtraction, rstd, gamma, beta and the residual: n_ops = 32 relative to
    |res| + |gamma| (|z| + mean|z|) rstd + |beta|."""
    from eqxvision_amd import _lib
    g = torch.Generator().manual_seed(M * 7 + C)
    gam = (1.0 + 0.3 * torch.randn(C, generator=g)).float()
    bet = (0.2 * torch.randn(C, generator=g)).float()
    res = torch.randn(M, C, generator=g).float()
    worst = 0.0
    for zdt in (torch.bfloat16, torch.float32):
        z = (1.7 * torch.randn(M, C, generator=g) + 0.3).to(zdt)
        z64 = z.double()
        mu = z64.mean(-1, keepdim=True)
        rstd = 1.0 / torch.sqrt(((z64 - mu) ** 2).mean(-1, keepdim=True) + 1e-5)
        nrm = (z64 - mu) * rstd * gam.double() + bet.double()
        nmag = gam.double().abs() * (z64.abs() + z64.abs().mean(-1, keepdim=True)) * rstd + bet.double().abs()
        for use_res in (True, False):
            ref = nrm + (res.double() if use_res else 0.0)
            mag = nmag + (res.double().abs() if use_res else 0.0)
            for use_lo in (True, False):
                y = _dest(M, C, torch.float32)
                lo = _dest(M, C, torch.bfloat16) if use_lo else None
                zd, rd, gd, bd = z.cuda(), res.cuda(), gam.cuda(), bet.cuda()
                _lib.call("mv_layernorm_add_fwd", _p(zd), _p(rd) if use_res else None, _p(gd), _p(bd), _p(y), _p(lo), M, C, 1e-5,
                          _lib.BF16 if zdt == torch.bfloat16 else _lib.F32, _lib.BF16, _stream())
                assert _lib.last_kernel() == "layernorm_add"
                torch.cuda.synchronize()
                yh = y.cpu()
                assert bool((yh[M * C:] == SENTINEL).all())
                got = yh[:M * C].reshape(M, C)
                info = ST.check_bound(got.double().numpy(), ref.numpy(), mag.numpy(), 0, "fp32", n_ops=32)
                assert info["ok"], (str(zdt), use_res, use_lo, info)
                worst = max(worst, info["worst"])
                if use_lo:
                    lh = lo.cpu()
                    assert bool((lh[M * C:].float() == SENTINEL).all())
                    assert torch.equal(lh[:M * C].reshape(M, C), got.to(torch.bfloat16)), "y_lo is not the RNE rounding of y"
    print(f"layernorm_add M={M} C={C}: worst {worst:.3f} of the bound")


# ------------------------------------------------------------------------------------------------ 4. fused against literal
def _rand_affines(model, seed):
    """Non-trivial LayerNorm affines and logit scales in [log 2, log 12]; everything else stays as constructed."""
    rng = np.random.Generator(np.random.PCG64(seed))
    from eqxvision_amd import nn as enn
    from eqxvision_amd._module import Module

    def rec(n):
        if isinstance(n, enn.LayerNorm) and n.weight is not None:
            object.__setattr__(n, "weight", (1.0 + 0.2 * rng.standard_normal(n.weight.shape)).astype(np.float32))
            object.__setattr__(n, "bias", (0.1 * rng.standard_normal(n.bias.shape)).astype(np.float32))
        if isinstance(n, Module):
            if hasattr(n, "logit_scale"):
                object.__setattr__(n, "logit_scale", rng.uniform(math.log(2.0), math.log(12.0), n.logit_scale.shape).astype(np.float32))
            for f in n.__fields__:
                if hasattr(n, f):
                    rec(getattr(n, f))
        elif isinstance(n, (list, tuple)):
            for c in n:
                rec(c)
    rec(model)
    return model


def _with_flag(name, value, fn):
    from eqxvision_amd import _lib
    _lib.set_flag(name, value)
    try:
        return fn()
    finally:
        _lib.set_flag(name, 0)


def test_block_and_merging_fused_vs_literal():
    """ops with "no_swin_v2_fused" off and on.  Both run the same GEMM and attention launches on the same operands; only
    mv_layernorm_add_fwd is swapped against LayerNorm + add, and the bf16 plane written next to the stream against the consumer's
    cast.  So the bound is far below the issue's (test 2's 2^-7 max|v| plus one bf16 rounding of the plane, asserted too, with
    max|v| taken from the data): the fp32 streams agree to 4 fp32 roundings of the row (the residual add, the affine, a
    contracted multiply-add), and the plane is bitwise the round-to-nearest-even of the stream it was written with."""
    from eqxvision_amd.models.classification import swin as S
    from eqxvision_amd._act import Act
    from eqxvision_amd import ops
    blk = _rand_affines(S._SwinTransformerBlockV2(96, 3, [8, 8], [4, 4], key=jr.PRNGKey(2)), 1)
    blk = eqv.tree_inference(blk, True)
    mrg = _rand_affines(S._PatchMergingV2(96, key=jr.PRNGKey(4)), 2)
    x = torch.randn(2, 16, 16, 96, generator=torch.Generator().manual_seed(0)).cuda()

    def run():
        a = blk(Act(x.clone(), "map", True))
        b = mrg(a)
        qkv = ops.linear(ops.stream_plane(Act(x.clone(), "map", True)), ops.swin_v2_qkv(blk.attn))
        torch.cuda.synchronize()
        planes = [None if t.pre is None else t.pre[1].t.cpu() for t in (a, b)]
        return a.t.cpu(), b.t.cpu(), planes, float(qkv.t[..., 192:].float().abs().max())
    fa, fb, fpl, vmax = run()
    la, lb, lpl, _ = _with_flag("no_swin_v2_fused", 1, run)
    assert lpl == [None, None] and all(p is not None for p in fpl)
    for tag, f, l, pl in (("block", fa, la, fpl[0]), ("merging", fb, lb, fpl[1])):
        err = float((f.double() - l.double()).abs().max())
        tight = 4 * 2.0 ** -23 * float(l.abs().max())
        issue = 2.0 ** -7 * vmax + 2.0 ** -9 * float(l.abs().max())
        print(f"fused vs literal {tag}: err {err:.3e} tight bound {tight:.3e} (the issue's bound {issue:.3e})")
        assert bool(torch.isfinite(f).all()) and err <= tight <= issue
        assert torch.equal(pl, f.to(torch.bfloat16)), "the bf16 plane is not the RNE rounding of the stream"


# ------------------------------------------------------------------------------------------------ 5. models against the restatement
def _reduced(seed, sd=0.0):
    from eqxvision_amd.models.classification.swin import SwinTransformer, _PatchMergingV2, _SwinTransformerBlockV2
    m = SwinTransformer([4, 4], 64, [2, 2], [2, 4], [8, 8], stochastic_depth_prob=sd, num_classes=10, block=_SwinTransformerBlockV2,
                        downsample_layer=_PatchMergingV2, key=jr.PRNGKey(seed))
    return _rand_affines(m, seed)


def _precise(C, depth):
    return C not in (96, 192, 384, 768) or depth > 6


def _image(B, px, seed):
    return torch.randn(B, 3, px, px, generator=torch.Generator().manual_seed(seed))


def _keys(B, seed=0):
    return eqv.random.split(eqv.random.PRNGKey(seed), B)


def _engine(model, x, mode, inference=True, keys=None):
    net = eqv.tree_inference(model, True) if inference else model
    with eqv.precision(mode):
        out = eqv.vmap(net, axis_name="batch")(x, key=_keys(x.shape[0]) if keys is None else keys)
    return out.cpu().double()


# d: max |restatement(emulate="bf16") - restatement(float64)| over the logits of the case, measured on the CPU with
# tests/_swin_v2_ref.py alone (the reduced model of _reduced(3) on _image(2, 128, 7)); the engine may deviate from float64 by 2 d
# (different summation orders, __expf).  Measured engine deviation on the MI355X: 4.23e-3, a margin of 1.56x.
D_REDUCED_128 = 3.294e-3


def test_reduced_model_fp32_well_conditioned():
    m = _reduced(3)
    x = _image(2, 128, 7)
    P = R.weights_of(m)
    ref = torch.stack([R.model(x[b].double(), P)[0] for b in range(2)])
    got = _engine(m, x, "fp32")
    err = float((got - ref).abs().max())
    print(f"reduced 128 px fp32: err {err:.3e} (tol {FP32_TOL})")
    assert err <= FP32_TOL


def test_reduced_model_bf16_well_conditioned():
    m = _reduced(3)
    x = _image(2, 128, 7)
    P = R.weights_of(m)
    ref = torch.stack([R.model(x[b].double(), P)[0] for b in range(2)])
    emu = torch.stack([R.model(x[b].double(), P, emulate="bf16", precise=_precise)[0] for b in range(2)])
    d = float((emu - ref).abs().max())
    assert abs(d - D_REDUCED_128) <= 0.01 * D_REDUCED_128, d                  # the recorded constant is this measurement
    got = _engine(m, x, "bf16")
    err = float((got - ref).abs().max())
    print(f"reduced 128 px bf16: d {d:.3e} err {err:.3e} margin {2 * d / max(err, 1e-30):.2f}x")
    assert err <= 2 * D_REDUCED_128


SEED_SINGLE = 3          # chosen on the CPU: the guard below holds for _reduced(SEED_SINGLE) on _image(1, 64, 7)


def test_reduced_model_fp32_single_window():
    """64 px: the last stage (8 x 8 map) has one window, q_hat = sign(q).  Guard, from the restatement alone: every |q| and |k|
    entering a single-window normalisation is at least 1e-5 of that tensor's rms."""
    m = _reduced(SEED_SINGLE)
    x = _image(1, 64, 7)
    ref, stats = R.model(x[0].double(), R.weights_of(m))
    assert stats
    for q, k in stats:
        for t in (q, k):
            assert float(t.min()) >= 1e-5 * float(torch.sqrt((t * t).mean())), "conditioning guard: pick another seed"
    got = _engine(m, x, "fp32")[0]
    err = float((got - ref).abs().max())
    print(f"reduced 64 px fp32 (single window): err {err:.3e} (tol {FP32_TOL})")
    assert err <= FP32_TOL


def test_swin_v2_t_256_bf16_shape_finite_and_replay():
    """What the reference's own test asserts at 256 px (tests/test_models/test_swin.py:12-23), and the filter_jit replay with two
    lanes is bit-identical to the eager call."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = eqv.tree_inference(eqv.models.swin_v2_t(), True)
    x = _image(1, 256, 1)
    with eqv.precision("bf16"):
        eager = eqv.vmap(m, axis_name="batch")(x, key=_keys(1)).cpu().numpy()
        assert eager.shape == (1, 1000) and np.isfinite(eager).all()
        fwd = eqv.filter_jit(lambda n, im, k: eqv.vmap(n, axis_name="batch")(im, key=k), lanes=2)
        outs = [fwd(m, x, _keys(1)).cpu().numpy() for _ in range(3)]              # the recording, then two replays
    for o in outs:
        assert np.array_equal(o, eager)


# ------------------------------------------------------------------------------------------------ factory size, training mode, dropout rates
# Every d below: max |restatement(emulate="bf16") - restatement(float64)| over the case's outputs, measured on the CPU with
# tests/_swin_v2_ref.py alone; the engine may deviate from float64 by 2 d.  The margins are the MI355X measurements.
D_T_512 = 1.2239e-2          # swin_v2_t, 512 px: 2 d = 2.4e-2 is ABOVE the project's 1e-2 bar; the case is not shrunk
D_TRAIN_128 = 3.7945e-3      # _reduced(3, sd=0.5) on _image(2, 128, 7), keys _keys(2, seed=11), logits
D_BLOCK_DROP = 1.3594e-1     # one block (C = 64, 16 x 16 map, shift 4) with attention_dropout 0.25 / dropout 0.1: the block's OUTPUT rows (max |.| ~ 5), not logits
SEED_T_256 = 9               # image seed chosen on the CPU (seeds 1 .. 9 tried: 1, 5, 6 and 9 hold): guard 2.16e-5 >= 1e-5
_CACHE = {}


def _factory():
    """swin_v2_t with non-trivial affines and logit scales, its restatement weights, and the float64 references (computed once)."""
    if "m" not in _CACHE:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            _CACHE["m"] = _rand_affines(eqv.models.swin_v2_t(), 5)
        _CACHE["P"] = R.weights_of(_CACHE["m"])
    return _CACHE["m"], _CACHE["P"]


def _factory_ref(px, seed):
    if ("ref", px) not in _CACHE:
        _, P = _factory()
        _CACHE[("ref", px)] = R.model(_image(1, px, seed)[0].double(), P)
    return _CACHE[("ref", px)]


def test_swin_v2_t_512_fp32():
    """The factory at 512 px: 256 / 64 / 16 / 4 windows per image, every stage well conditioned."""
    m, _ = _factory()
    ref, stats = _factory_ref(512, 7)
    assert not stats                                                        # no single-window stage
    got = _engine(m, _image(1, 512, 7), "fp32")[0]
    err = float((got - ref).abs().max())
    print(f"swin_v2_t 512 px fp32: err {err:.3e} (tol {FP32_TOL}), max|logit| {float(ref.abs().max()):.2f}")
    assert err <= FP32_TOL


def test_swin_v2_t_512_bf16():
    m, P = _factory()
    ref, _ = _factory_ref(512, 7)
    emu, _ = R.model(_image(1, 512, 7)[0].double(), P, emulate="bf16", precise=_precise)
    d = float((emu - ref).abs().max())
    assert abs(d - D_T_512) <= 0.01 * D_T_512, d
    got = _engine(m, _image(1, 512, 7), "bf16")[0]
    err = float((got - ref).abs().max())
    print(f"swin_v2_t 512 px bf16: d {d:.3e} err {err:.3e} margin {2 * d / max(err, 1e-30):.2f}x")
    assert err <= 2 * D_T_512


def test_swin_v2_t_256_fp32_single_window():
    """256 px, the reference test's own size: the last stage has one window.  fp32 only, behind the conditioning guard."""
    m, _ = _factory()
    ref, stats = _factory_ref(256, SEED_T_256)
    assert len(stats) == 2
    for q, k in stats:
        for t in (q, k):
            assert float(t.min()) >= 1e-5 * float(torch.sqrt((t * t).mean())), "conditioning guard: pick another seed"
    got = _engine(m, _image(1, 256, SEED_T_256), "fp32")[0]
    err = float((got - ref).abs().max())
    print(f"swin_v2_t 256 px fp32 (single-window last stage): err {err:.3e} (tol {FP32_TOL})")
    assert err <= FP32_TOL


def _sd_drops(model, key):
    """The stochastic-depth scales of ONE sample on the reference's key schedule: the model splits its key in two (:766), `features`
    (nn.Sequential) over its layers, a stage over its blocks, a block in four (:630); DropPath "local" draws one value per channel
    of the (C, H, W) sample (drop_path.py:55-60)."""
    L = model.features.layers
    ks = jr.split(jr.split(key, 2)[0], len(L))
    drops, bi = {}, 0
    for i in range(1, len(L), 2):
        kk = jr.split(ks[i], len(L[i].layers))
        for j, b in enumerate(L[i].layers):
            k4, p = jr.split(kk[j], 4), b.stochastic_depth.p
            if p > 0:
                C = b.norm1.shape[0]
                drops[bi] = {n: R.t64(jr.bernoulli(k4[w], 1.0 - p, (C,))) / (1.0 - p) for n, w in (("sd1", 1), ("sd2", 3))}
            bi += 1
    return drops


def test_reduced_model_training_mode_bf16():
    """Training mode (no tree_inference), stochastic depth 0.5 (block rates 0, 1/6, 1/3, 1/2), the literal composition."""
    m = _reduced(3, sd=0.5)
    x = _image(2, 128, 7)
    keys = _keys(2, seed=11)
    P = R.weights_of(m)
    drops = [_sd_drops(m, keys[b]) for b in range(2)]
    assert sorted(drops[0]) == [1, 2, 3] and any(float(v.min()) == 0 for d_ in drops for bd in d_.values() for v in bd.values())
    ref = torch.stack([R.model(x[b].double(), P, drops=drops[b])[0] for b in range(2)])
    emu = torch.stack([R.model(x[b].double(), P, emulate="bf16", precise=_precise, drops=drops[b])[0] for b in range(2)])
    d = float((emu - ref).abs().max())
    assert abs(d - D_TRAIN_128) <= 0.01 * D_TRAIN_128, d
    got = _engine(m, x, "bf16", inference=False, keys=keys)
    err = float((got - ref).abs().max())
    print(f"reduced 128 px bf16 training mode: d {d:.3e} err {err:.3e} margin {2 * d / max(err, 1e-30):.2f}x")
    assert err <= 2 * D_TRAIN_128


def test_block_with_dropout_rates_bf16():
    """attention_dropout = 0.25 and dropout = 0.1 drop in EVERY mode (swin.py:17-20): both draws use the block's first key (:227,
    :233), on the shapes (nW, heads, n, n) and (nW, n, C) of the shifted, partitioned map."""
    from eqxvision_amd.models.classification import swin as S
    from eqxvision_amd._act import Act
    pa, pd = 0.25, 0.1
    blk = _rand_affines(S._SwinTransformerBlockV2(64, 2, [8, 8], [4, 4], dropout=pd, attention_dropout=pa, key=jr.PRNGKey(6)), 3)
    blk = eqv.tree_inference(blk, True)                                     # the MLP's nn.Dropout is off; _func_dropout is not
    x = torch.randn(1, 16, 16, 64, generator=torch.Generator().manual_seed(1))
    key = jr.PRNGKey(8)
    k0 = jr.split(key, 4)[0]
    drop = {"attn": R.t64(jr.bernoulli(k0, 1.0 - pa, (4, 2, 64, 64))) / (1.0 - pa),
            "proj": R.t64(jr.bernoulli(k0, 1.0 - pd, (4, 64, 64))) / (1.0 - pd)}
    a = blk.attn
    lins = [l for l in a.cpb_mlp.layers if hasattr(l, "weight")]
    bp = {"qkv.weight": a.qkv.weight, "qkv.bias": a.qkv.bias, "proj.weight": a.proj.weight, "proj.bias": a.proj.bias,
          "logit_scale": a.logit_scale, "norm1.weight": blk.norm1.weight, "norm1.bias": blk.norm1.bias, "norm2.weight": blk.norm2.weight,
          "norm2.bias": blk.norm2.bias, "fc1.weight": blk.mlp.fc1.weight, "fc1.bias": blk.mlp.fc1.bias, "fc2.weight": blk.mlp.fc2.weight,
          "fc2.bias": blk.mlp.fc2.bias}
    bp = {k: R.t64(v) for k, v in bp.items()}
    bp.update({"table": np.asarray(a.relative_position_bias_table), "index": np.asarray(a.relative_position_index),
               "cpb.w1": np.asarray(lins[0].weight), "cpb.b1": np.asarray(lins[0].bias), "cpb.w2": np.asarray(lins[1].weight)})
    ref = R.block(x[0].double(), bp, 2, [8, 8], [4, 4], drop=drop)
    emu = R.block(x[0].double(), bp, 2, [8, 8], [4, 4], emulate="bf16", split=True, drop=drop)
    d = float((emu - ref).abs().max())
    assert abs(d - D_BLOCK_DROP) <= 0.01 * D_BLOCK_DROP, d
    with eqv.precision("bf16"):
        y = blk(Act(x.cuda(), "map", True), key=key[None])
    torch.cuda.synchronize()
    got = y.t[0].double().cpu()
    err = float((got - ref).abs().max())
    print(f"block with dropout rates bf16: d {d:.3e} err {err:.3e} margin {2 * d / max(err, 1e-30):.2f}x")
    assert bool(torch.isfinite(got).all()) and err <= 2 * D_BLOCK_DROP


def test_filter_value_and_grad_raises():
    """Through the public transform: the model refuses before anything of V2 is launched (the backward is not built)."""
    m = _reduced(3)

    @eqv.filter_value_and_grad
    def loss(model, x):
        out = eqv.vmap(model, axis_name="batch")(x, key=_keys(1))
        return out.sum()

    with pytest.raises(NotImplementedError, match="without a backward"):
        loss(m, _image(1, 64, 7))
