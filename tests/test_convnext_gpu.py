"""`-m gpu`: ConvNeXt on the MI355X -- the 7x7 depthwise + LayerNorm kernel and the residual-from-another-tensor MLP entries
against torch-fp64 references, and whole networks (loaded through `torch_weights=`) against the restatement in
tests/_convnext_ref.py.  Margins are printed (`pytest -s`)."""
import os
import tempfile
import warnings

import numpy as np
import pytest
import torch

import eqxvision_amd as eqv
from oracle import state as S
from tests import _convnext_ref as R

pytestmark = pytest.mark.gpu

BF16_TOL, FP32_TOL = 1e-2, 1e-3


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from eqxvision_amd import _lib
    _lib.load()
    _lib.check_device_status()
    yield
    _lib.check_device_status()


def _p(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------------------------------------ op level: mv_cnblock_dw_fwd
DW_CASES = [(C, hw, B) for C in (96, 128, 192, 384, 768, 1024, 1536, 8 * 13)
            for hw, B in (((56, 56), 1), ((28, 28), 3), ((14, 14), 1), ((7, 7), 3), ((5, 5), 1), ((9, 13), 3))
            if not (C >= 768 and hw == (56, 56)) and not (C >= 1024 and hw == (28, 28))]


def _dw_ref(x, w, b, normalize, eps):
    xd = x.double().permute(0, 3, 1, 2)
    C = xd.shape[1]
    d = torch.nn.functional.conv2d(xd, w.double().permute(2, 0, 1).reshape(C, 1, 7, 7), b.double(), padding=3, groups=C)
    d = d.permute(0, 2, 3, 1)
    if normalize:
        m = d.mean(-1, keepdim=True)
        d = (d - m) / torch.sqrt(((d - m) ** 2).mean(-1, keepdim=True) + eps)
    return d


@pytest.mark.parametrize("C,hw,B", DW_CASES, ids=[f"C{c}_{h}x{w}_B{b}" for c, (h, w), b in DW_CASES])
def test_cnblock_dw(C, hw, B):
    from eqxvision_amd import _lib
    H, W = hw
    g = torch.Generator().manual_seed(C * 1000 + H * 10 + B)
    x32 = torch.randn(B, H, W, C, generator=g)
    w = (torch.randn(7, 7, C, generator=g) * 0.15).to(torch.bfloat16)
    b = torch.randn(C, generator=g) * 0.1
    wd, bd = w.cuda(), b.cuda()
    eps = 1e-5
    for x_dt, xt in ((_lib.F32, x32), (_lib.BF16, x32.to(torch.bfloat16))):
        xd = xt.cuda()
        for normalize, y_dt in ((0, _lib.BF16), (0, _lib.F32), (1, _lib.BF16)):
            assert _lib.load().mv_cnblock_dw_supported(C, H, W, x_dt, y_dt, normalize)
            y = torch.empty(B, H, W, C, dtype=torch.float32 if y_dt == _lib.F32 else torch.bfloat16, device="cuda")
            _lib.call("mv_cnblock_dw_fwd", _p(xd), _p(wd), _p(bd), _p(y), B, H, W, C, eps, normalize, x_dt, y_dt, _stream())
            ref = _dw_ref(xt.float(), w.float(), b, normalize, eps)
            err = float((y.double().cpu() - ref).abs().max())
            scale = float(ref.abs().max())
            bound = (2.0 ** -8 if y_dt == _lib.BF16 else 1e-5) * scale
            assert err <= bound, (x_dt, normalize, y_dt, err, scale)


def test_cnblock_dw_large_offset():
    """Rows whose mean is far above their spread: the two-pass statistics keep the normalised values."""
    from eqxvision_amd import _lib
    B, H, W, C = 2, 14, 14, 384
    g = torch.Generator().manual_seed(7)
    x = torch.randn(B, H, W, C, generator=g) + 300.0 * torch.rand(B, H, W, 1, generator=g) + 100.0
    w = (torch.full((7, 7, C), 1.0 / 49) + 0.01 * torch.randn(7, 7, C, generator=g)).to(torch.bfloat16)
    b = torch.zeros(C)
    y = torch.empty(B, H, W, C, dtype=torch.bfloat16, device="cuda")
    xd, wd, bd = x.cuda(), w.cuda(), b.cuda()                          # alive until the launch has run
    _lib.call("mv_cnblock_dw_fwd", _p(xd), _p(wd), _p(bd), _p(y), B, H, W, C, 1e-5, 1, _lib.F32, _lib.BF16, _stream())
    ref = _dw_ref(x, w.float(), b, 1, 1e-5)
    err = float((y.double().cpu() - ref).abs().max())
    assert err <= 2.0 ** -8 * float(ref.abs().max()), err


# ------------------------------------------------------------------------------------------------ op level: the _res MLP entries
MLP_CASES = [(96, 3136), (96, 200704), (192, 784), (192, 50176), (384, 196), (384, 12544)]


def _mlp_weights(C, seed):
    from eqxvision_amd import ops
    g = np.random.default_rng(seed)
    Hd = 4 * C
    w1 = g.uniform(-1, 1, (Hd, C)).astype(np.float32) / np.sqrt(C)
    b1 = g.uniform(-0.1, 0.1, Hd).astype(np.float32)
    w2 = g.uniform(-1, 1, (C, Hd)).astype(np.float32) / np.sqrt(Hd)
    b2 = g.uniform(-0.1, 0.1, C).astype(np.float32)
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt).cuda()
    if C == 96:
        return (dev(w1, torch.bfloat16), dev(b1, torch.float32), dev(w2, torch.bfloat16), dev(b2, torch.float32)), (w1, b1, w2, b2)
    f1, f2 = ops.ln_mlp_fragments(w1, w2)
    return (dev(f1, torch.bfloat16), dev(b1, torch.float32), dev(f2, torch.bfloat16), dev(b2, torch.float32)), (w1, b1, w2, b2)


@pytest.mark.parametrize("C,M", MLP_CASES, ids=[f"C{c}_M{m}" for c, m in MLP_CASES])
def test_ln_mlp_res(C, M):
    from eqxvision_amd import _lib
    dev_w, (w1, b1, w2, b2) = _mlp_weights(C, C + M)
    g = torch.Generator().manual_seed(M)
    d = torch.randn(M, C, generator=g) * 2.0 + 0.5
    res = torch.randn(M, C, generator=g) * 3.0
    lds = C == 96
    entry, xdt = ("mv_ln_mlp_res_fwd", _lib.BF16) if lds else ("mv_ln_mlp_stream_res_fwd", _lib.F32)
    xd = d.to(torch.bfloat16) if lds else d
    y = torch.empty(M, C, dtype=torch.float32, device="cuda")
    xg, rg = xd.cuda(), res.cuda()
    _lib.call(entry, _p(xg), _p(rg), *[_p(t) for t in dev_w], _p(y), M, C, 4 * C, 1e-5, xdt, _stream())
    # reference: fp64 with the device's bf16 weights
    xr = xd.double().cuda()
    n = (xr - xr.mean(-1, keepdim=True)) / torch.sqrt(xr.var(-1, unbiased=False, keepdim=True) + 1e-5)
    bf = lambda a: torch.from_numpy(a).to(torch.bfloat16).double().cuda()
    h = torch.nn.functional.gelu(n @ bf(w1).T + torch.from_numpy(b1).double().cuda(), approximate="tanh")
    mlp = h @ bf(w2).T + torch.from_numpy(b2).double().cuda()
    ref = res.double().cuda() + mlp
    err = float((y.double() - ref).abs().max())
    assert err <= 2e-2 * float(mlp.abs().max()), (err, float(mlp.abs().max()))
    # res = x on an fp32 x: bit for bit the entry without _res (the existing path is untouched)
    x32 = d.cuda()
    y_old = torch.empty_like(y)
    y_new = torch.empty_like(y)
    old = "mv_ln_mlp_fwd" if lds else "mv_ln_mlp_stream_fwd"
    _lib.call(old, _p(x32), *[_p(t) for t in dev_w], _p(y_old), M, C, 4 * C, 1e-5, _lib.F32, _stream())
    _lib.call(entry, _p(x32), _p(x32), *[_p(t) for t in dev_w], _p(y_new), M, C, 4 * C, 1e-5, _lib.F32, _stream())
    assert torch.equal(y_old, y_new)


# ------------------------------------------------------------------------------------------------ model level
def _net(arch, sd, **kw):
    with tempfile.TemporaryDirectory() as td:
        p = os.path.join(td, "w.pth")
        S.save_pth(sd, p)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return getattr(eqv.models, arch)(torch_weights=p, **kw)


def _keys(B, seed=0):
    return eqv.random.split(eqv.random.PRNGKey(seed), B)


def _run(net, x, keys=None, dtype="bf16"):
    with eqv.precision(dtype):
        return eqv.vmap(net, axis_name="batch")(x, key=keys if keys is not None else _keys(x.shape[0])).cpu().numpy()


def _margins(got, ref, tol):
    err = float(np.abs(got - ref).max())
    scale = max(1.0, float(np.abs(ref).max()))
    info = {"err": err, "err_scaled": err / scale, "argmax_match": float((got.argmax(-1) == ref.argmax(-1)).mean()),
            "max_ref": float(np.abs(ref).max())}
    print(info)
    return err <= tol, info


_CACHE = {}


def _case(arch, B, size=224, seed=1):
    key = (arch, B, size, seed)
    if key not in _CACHE:
        sd = R.convnext_state(R.SETTINGS[arch], seed=seed)
        x = S.synthetic_images(B, size, seed=seed)
        ref = R.forward_torch(sd, R.SETTINGS[arch], x, device="cuda")
        _CACHE[key] = (sd, x, ref)
    return _CACHE[key]


def test_tiny_bf16_fp32_and_layer_scale_matters():
    sd, x, ref = _case("convnext_tiny", 2)
    net = eqv.tree_inference(_net("convnext_tiny", sd), True)
    xt = torch.as_tensor(x).cuda()
    ok, info = _margins(_run(net, xt), ref, BF16_TOL)
    assert ok, info
    assert 0.5 <= info["max_ref"] <= 3.0, info
    ok, info = _margins(_run(net, xt, dtype="fp32"), ref, FP32_TOL)
    assert ok, info
    sd0 = {k: (np.zeros_like(v) if k.endswith("layer_scale") else v) for k, v in sd.items()}
    ref0 = R.forward_torch(sd0, R.SETTINGS["convnext_tiny"], x, device="cuda")
    assert float(np.abs(ref0 - ref).max()) > 10 * BF16_TOL


def test_tiny_fused_vs_switches_off():
    from eqxvision_amd import _lib
    sd, x, ref = _case("convnext_tiny", 2)
    net = eqv.tree_inference(_net("convnext_tiny", sd), True)
    xt = torch.as_tensor(x).cuda()
    on = _run(net, xt)
    flags = ("no_cnblock_dw", "no_ln_mlp", "no_ln_mlp_stream")
    for f in flags:
        _lib.set_flag(f, 1)
    try:
        off = _run(net, xt)
    finally:
        for f in flags:
            _lib.set_flag(f, 0)
    for got in (on, off):
        ok, info = _margins(got, ref, BF16_TOL)
        assert ok, info
    assert not np.array_equal(on, off)


def test_tiny_b64_lanes_replay():
    sd, x, ref = _case("convnext_tiny", 64, seed=2)
    net = eqv.tree_inference(_net("convnext_tiny", sd), True)
    xt = torch.as_tensor(x).cuda()
    eager = _run(net, xt)

    def body(n, im, k):
        return eqv.vmap(n, axis_name="batch")(im, key=k)

    fwd = eqv.filter_jit(body, lanes=2)
    with eqv.precision("bf16"):
        outs = [fwd(net, xt, _keys(64)).cpu().numpy() for _ in range(3)]
    # a lane is an eager forward of its half of the batch (the few-row Linears of stage 3 may split K differently at 32 than at 64)
    halves = np.concatenate([_run(net, xt[:32].contiguous()), _run(net, xt[32:].contiguous())])
    for o in outs:
        assert np.array_equal(o, halves)
    for got in (outs[0], eager):
        ok, info = _margins(got, ref, BF16_TOL)
        assert ok, info


@pytest.mark.parametrize("arch,B", [("convnext_small", 2), ("convnext_base", 1), ("convnext_large", 1)])
def test_bigger_nets_bf16(arch, B):
    sd, x, ref = _case(arch, B)
    net = eqv.tree_inference(_net(arch, sd), True)
    ok, info = _margins(_run(net, torch.as_tensor(x).cuda()), ref, BF16_TOL)
    assert ok, info


def test_tiny_training_mode_masks():
    sd, x, _ = _case("convnext_tiny", 2)
    setting = R.SETTINGS["convnext_tiny"]
    net = _net("convnext_tiny", sd, stochastic_depth_prob=0.5)
    keys = _keys(2, seed=9)
    masks = R.training_masks(setting, keys, 0.5)
    ref = R.forward_torch(sd, setting, x, masks, device="cuda")
    ok, info = _margins(_run(net, torch.as_tensor(x).cuda(), keys=keys), ref, BF16_TOL)
    assert ok, info
    plain = R.forward_torch(sd, setting, x, device="cuda")
    assert float(np.abs(plain - ref).max()) > 10 * BF16_TOL             # the masks matter


def test_grad_refuses():
    m = eqv.models.convnext_tiny(num_classes=3)

    @eqv.filter_value_and_grad
    def loss(model, x, y):
        out = eqv.vmap(model, axis_name="batch")(x, key=_keys(1))
        return eqv.optim.softmax_cross_entropy(out, eqv.optim.one_hot(y, 3)).mean()

    with pytest.raises(NotImplementedError, match="without a backward"):
        loss(m, torch.zeros((1, 3, 32, 32), device="cuda"), np.zeros((1,), np.int32))
