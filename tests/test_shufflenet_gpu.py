"""`-m gpu`: ShuffleNetV2 on the MI355X -- the fused depthwise + 1x1 + pass-through kernel against a torch-fp64 reference and against
the two-launch composition it replaces, the channel gather, and whole networks (loaded through `torch_weights=`) against the
restatement in tests/_shufflenet_ref.py.  Margins are printed (`pytest -s`)."""
import os
import tempfile
import warnings

import numpy as np
import pytest
import torch

import eqxvision_amd as eqv
from oracle import state as S
from tests import _shufflenet_ref as R

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


# ------------------------------------------------------------------------------------------------ op level: mv_shuffle_dwpw_fwd
def _triples():
    """Every (Cx, N, N_real, hw of the launch's input, stride) the four factories produce at a 224 input."""
    from eqxvision_amd import ops
    out = []
    for _, widths in R.SETTINGS.values():
        hw, cphys = 56, widths[0]
        for cout in widths[1:4]:
            bf, P = ops.shuffle_layout(cout // 2)
            out += [(cphys, P, bf, hw, 2), (P, P, bf, hw, 2), (P, P, bf, hw // 2, 1)]
            hw, cphys = hw // 2, 2 * P
    seen, uniq = set(), []
    for t in out:
        if t not in seen:
            seen.add(t)
            uniq.append(t)
    return uniq


DWPW_CASES = _triples()
SENTINEL = -7.0


def _dwpw_ref(x, wdw, ds, dh, wpw, ps, ph, stride):
    """fp64 on the bf16-rounded operands, the depthwise result NOT rounded."""
    C = x.shape[-1]
    d = torch.nn.functional.conv2d(x.double().permute(0, 3, 1, 2), wdw.double().permute(2, 0, 1).reshape(C, 1, 3, 3), stride=stride,
                                   padding=1, groups=C).permute(0, 2, 3, 1)
    d = d * ds.double() + dh.double()
    return torch.relu(d @ wpw.double().T * ps.double() + ph.double())


def _one_dwpw(Cx, N, N_real, H, W, B, stride, with_pass, y_off, seed):
    from eqxvision_amd import _lib, ops
    lib = _lib.load()
    assert lib.mv_shuffle_dwpw_supported(Cx, N, stride, H, W, _lib.BF16, _lib.BF16) == 1
    g = torch.Generator().manual_seed(seed)
    dev = "cuda"
    x = torch.randn(B, H, W, Cx, generator=g).to(torch.bfloat16).to(dev)
    wdw = (torch.randn(3, 3, Cx, generator=g) * 0.4).to(torch.bfloat16).to(dev)
    ds = (torch.rand(Cx, generator=g) + 0.5).to(dev)
    dh = (torch.randn(Cx, generator=g) * 0.1).to(dev)
    wpw = torch.zeros(N, Cx)
    wpw[:N_real] = torch.randn(N_real, Cx, generator=g) / np.sqrt(Cx)
    wpw = wpw.to(torch.bfloat16)
    ps, ph = torch.zeros(N), torch.zeros(N)
    ps[:N_real] = torch.rand(N_real, generator=g) + 0.5
    ph[:N_real] = torch.randn(N_real, generator=g) * 0.1
    frag = torch.from_numpy(ops.dwpw_fragments(wpw.float().numpy())).to(torch.bfloat16).to(dev)
    wpw, ps, ph = wpw.to(dev), ps.to(dev), ph.to(dev)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    pitch = 2 * N
    y = torch.full((B, Ho, Wo, pitch), SENTINEL, dtype=torch.bfloat16, device=dev)
    pass_off = N - y_off                                   # the other half
    src = None
    pass_args = (None, 0, 0, 0, 0, 0)
    if with_pass:
        src = torch.randn(B, Ho, Wo, 2 * N, generator=g).to(torch.bfloat16).to(dev)
        pass_args = (_p(src), 2 * N, N, N_real, pass_off, N)
    _lib.call("mv_shuffle_dwpw_fwd", _p(x), _p(wdw), _p(ds), _p(dh), _p(frag), _p(ps), _p(ph), _p(y), pitch, y_off, N, N_real,
              *pass_args, B, H, W, Cx, stride, _lib.BF16, _lib.BF16, _stream())
    # the two-launch composition on the same device tensors (dense outputs)
    d = torch.empty(B, Ho, Wo, Cx, dtype=torch.bfloat16, device=dev)
    _lib.call("mv_dwconv2d_nhwc_fwd", _p(x), _p(wdw), _p(ds), _p(dh), _p(d), B, H, W, Cx, 3, 3, stride, stride, 1, 1, 1, 1, _lib.ACT_NONE,
              _lib.BF16, _lib.BF16, _stream())
    yc = torch.empty(B, Ho, Wo, N, dtype=torch.bfloat16, device=dev)
    _lib.call("mv_conv2d_nhwc_fwd", _p(d), _p(wpw), _p(ps), _p(ph), None, _p(yc), B, Ho, Wo, Cx, N, 1, 1, 1, 1, 0, 0, 1, 1, 1, _lib.ACT_RELU,
              _lib.BF16, _lib.BF16, _stream())
    torch.cuda.synchronize()
    ref = _dwpw_ref(x, wdw, ds, dh, wpw[:N_real], ps[:N_real], ph[:N_real], stride)
    scale = float(ref.abs().max())
    err_f = float((y[..., y_off:y_off + N_real].double() - ref).abs().max())
    err_c = float((yc[..., :N_real].double() - ref).abs().max())
    tag = dict(Cx=Cx, N=N, N_real=N_real, hw=(H, W), B=B, stride=stride, with_pass=with_pass, y_off=y_off)
    print({**tag, "err_fused": err_f, "err_composition": err_c, "max_ref": scale})
    assert err_f <= max(2.0 * err_c, 2.0 ** -8 * scale), (tag, err_f, err_c, scale)
    assert bool((y[..., y_off + N_real:y_off + N] == 0).all()), tag                      # pads: exact zeros
    other = y[..., pass_off:pass_off + N]
    if with_pass:
        idx = torch.from_numpy(ops.shuffle_phys_index(2 * N_real, (N_real, N))[:N_real]).to(dev)
        assert torch.equal(other[..., :N_real].view(torch.int16), src[..., idx].view(torch.int16)), tag    # bit copy
        assert bool((other[..., N_real:] == 0).all()), tag
    else:
        assert bool((other == SENTINEL).all()), tag                                       # untouched


@pytest.mark.parametrize("Cx,N,N_real,hw,stride", DWPW_CASES, ids=[f"Cx{a}_N{b}_{c}_{d}x{d}_s{e}" for a, b, c, d, e in DWPW_CASES])
def test_shuffle_dwpw(Cx, N, N_real, hw, stride):
    seed = Cx * 1000 + N + stride
    for B in (1, 3):                                       # the factory's own shape: with the pass-through where the network has it
        _one_dwpw(Cx, N, N_real, hw, hw, B, stride, stride == 1 and Cx == N, N if Cx == N else 0, seed + B)
    _one_dwpw(Cx, N, N_real, hw, hw, 1, stride, False, 0 if Cx == N else N, seed + 5)
    _one_dwpw(Cx, N, N_real, 9, 13, 1, 1, True, N, seed + 6)
    _one_dwpw(Cx, N, N_real, 9, 13, 3, 2, False, 0, seed + 7)
    _one_dwpw(Cx, N, N_real, 5, 5, 3, 1, False, N, seed + 8)
    _one_dwpw(Cx, N, N_real, 5, 5, 1, 2, False, 0, seed + 9)
    _one_dwpw(Cx, N, N_real, 5, 5, 3, 1, True, 0, seed + 10)


@pytest.mark.parametrize("hw", [56, 28, 14, 7])
def test_shuffle_dwpw_sizes_both_strides(hw):
    for stride in (1, 2):
        _one_dwpw(120, 120, 116, hw, hw, 3, stride, stride == 1, 120, hw + stride)


@pytest.mark.parametrize("C", [48, 116, 244])
def test_channel_gather(C):
    from eqxvision_amd import _lib
    g = torch.Generator().manual_seed(C)
    idx = torch.randperm(C, generator=g)[:C - 3].to(torch.int32)
    for dt, code in ((torch.bfloat16, _lib.BF16), (torch.float32, _lib.F32)):
        x = torch.randn(3, 9, 13, C, generator=g).to(dt).cuda()
        y = torch.empty(3, 9, 13, C - 3, dtype=dt, device="cuda")
        idx_d = idx.cuda()
        _lib.call("mv_channel_gather_nhwc_fwd", _p(x), _p(idx_d), _p(y), 3 * 9 * 13, C, C - 3, code, _stream())
        assert torch.equal(y, x[..., idx_d.long()])


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


def _run(net, x, dtype="bf16"):
    with eqv.precision(dtype):
        return eqv.vmap(net, axis_name="batch")(x, key=_keys(x.shape[0])).cpu().numpy()


def _margins(got, ref, tol):
    err = float(np.abs(got - ref).max())
    info = {"err": err, "argmax_match": float((got.argmax(-1) == ref.argmax(-1)).mean()), "max_ref": float(np.abs(ref).max())}
    print(info)
    return err <= tol, info


_CACHE = {}


def _case(arch, B, seed=1, **kw):
    key = (arch, B, seed, tuple(sorted(kw.items())))
    if key not in _CACHE:
        sd = R.shufflenet_state(R.SETTINGS[arch], seed=seed)
        x = S.synthetic_images(B, 224, seed=seed)
        _CACHE[key] = (sd, x, R.forward_torch(sd, R.SETTINGS[arch], x, device="cuda", **kw))
    return _CACHE[key]


@pytest.mark.parametrize("arch", ["shufflenet_v2_x0_5", "shufflenet_v2_x1_0"])
def test_bf16_and_fp32(arch):
    sd, x, ref = _case(arch, 2)
    net = eqv.tree_inference(_net(arch, sd), True)
    xt = torch.as_tensor(x).cuda()
    ok, info = _margins(_run(net, xt), ref, BF16_TOL)
    assert ok, info
    assert 0.5 <= info["max_ref"] <= 3.0, info
    ok, info = _margins(_run(net, xt, dtype="fp32"), ref, FP32_TOL)
    assert ok, info


@pytest.mark.parametrize("arch", ["shufflenet_v2_x1_5", "shufflenet_v2_x2_0"])
def test_wider_nets_bf16(arch):
    sd, x, ref = _case(arch, 1)
    net = eqv.tree_inference(_net(arch, sd), True)
    ok, info = _margins(_run(net, torch.as_tensor(x).cuda()), ref, BF16_TOL)
    assert ok, info


def test_fused_vs_switch_off():
    from eqxvision_amd import _lib
    sd, x, ref = _case("shufflenet_v2_x1_0", 2)
    net = eqv.tree_inference(_net("shufflenet_v2_x1_0", sd), True)
    xt = torch.as_tensor(x).cuda()
    on = _run(net, xt)
    _lib.set_flag("no_shuffle_dwpw", 1)
    try:
        off = _run(net, xt)
    finally:
        _lib.set_flag("no_shuffle_dwpw", 0)
    for got in (on, off):
        ok, info = _margins(got, ref, BF16_TOL)
        assert ok, info
    assert not np.array_equal(on, off)


def test_x1_0_b64_lanes_replay():
    sd, x, ref = _case("shufflenet_v2_x1_0", 64, seed=2)
    net = eqv.tree_inference(_net("shufflenet_v2_x1_0", sd), True)
    xt = torch.as_tensor(x).cuda()
    eager = _run(net, xt)

    def body(n, im, k):
        return eqv.vmap(n, axis_name="batch")(im, key=k)

    fwd = eqv.filter_jit(body, lanes=2)
    with eqv.precision("bf16"):
        outs = [fwd(net, xt, _keys(64)).cpu().numpy() for _ in range(3)]
    halves = np.concatenate([_run(net, xt[:32].contiguous()), _run(net, xt[32:].contiguous())])    # a lane = an eager half batch
    for o in outs:
        assert np.array_equal(o, halves)
    for got in (outs[0], eager):
        ok, info = _margins(got, ref, BF16_TOL)
        assert ok, info


def test_x0_5_training_mode_fp32():
    sd, x, ref = _case("shufflenet_v2_x0_5", 4, train_bn=True)
    net = _net("shufflenet_v2_x0_5", sd)                               # not through tree_inference: every BatchNorm trains
    ok, info = _margins(_run(net, torch.as_tensor(x).cuda(), dtype="fp32"), ref, FP32_TOL)
    assert ok, info
    plain = R.forward_torch(sd, R.SETTINGS["shufflenet_v2_x0_5"], x, device="cuda")
    assert float(np.abs(plain - ref).max()) > 0.0                       # the batch statistics entered


def test_grad_refuses():
    m = eqv.models.shufflenet_v2_x0_5(num_classes=3)

    @eqv.filter_value_and_grad
    def loss(model, x, y):
        out = eqv.vmap(model, axis_name="batch")(x, key=_keys(1))
        return eqv.optim.softmax_cross_entropy(out, eqv.optim.one_hot(y, 3)).mean()

    with pytest.raises(NotImplementedError, match="without a backward"):
        loss(m, torch.zeros((1, 3, 32, 32), device="cuda"), np.zeros((1,), np.int32))
