"""`-m gpu`: SqueezeNet on the MI355X -- the fused Fire expand kernel against fp64 convolutions on the same bf16-rounded operands and
against exact integers, the ceil-mode max pooling against torch, and whole networks (loaded through `torch_weights=`) against the
restatement in tests/_squeezenet_ref.py.  Margins are printed (`pytest -s`)."""
import os
import tempfile
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

import eqxvision_amd as eqv
from oracle import state as S
from tests import _squeezenet_ref as R
from tests._slices import GUARD, SENTINEL, _p, _stream

pytestmark = pytest.mark.gpu

BF16_TOL, FP32_TOL = 1e-2, 1e-3
MAPS = ((13, 13, 2), (5, 7, 3), (27, 27, 1), (1, 1, 2))     # (H, W, B): a few tiles; every pixel on a border; not a tile multiple; 1 pixel


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from eqxvision_amd import _lib
    _lib.load()
    _lib.check_device_status()
    yield
    _lib.check_device_status()


# ------------------------------------------------------------------------------------------------ op level: mv_fire_expand_fwd
def _launch_fire(t, w1, b1, w3, b3, wide):
    """-> (y [B, H, W, E1 + E3] on the host as float32, the guard behind it, the kernel's name)."""
    from eqxvision_amd import _lib, ops
    B, H, W, S_ = t.shape
    E1, E3 = w1.shape[0], w3.shape[0]
    assert _lib.load().mv_fire_expand_supported(S_, E1, E3, H, W, _lib.BF16, _lib.BF16) == 1
    f1 = torch.from_numpy(ops.fire_fragments(w1.float().numpy())).to(torch.bfloat16).cuda()
    f3 = torch.from_numpy(ops.fire_fragments(w3.float().numpy())).to(torch.bfloat16).cuda()
    n = B * H * W * (E1 + E3)
    buf = torch.full((n + GUARD,), SENTINEL, dtype=torch.bfloat16, device="cuda")
    td, b1d, b3d = t.cuda(), None if b1 is None else b1.cuda(), None if b3 is None else b3.cuda()
    if wide:
        _lib.set_flag("fire_expand_m256", 1)
    try:
        _lib.call("mv_fire_expand_fwd", _p(td), _p(f1), _p(b1d), _p(f3), _p(b3d), _p(buf), B, H, W, S_, E1, E3, _lib.BF16, _lib.BF16,
                  _stream())
        kern = _lib.last_kernel()
    finally:
        if wide:
            _lib.set_flag("fire_expand_m256", 0)
    torch.cuda.synchronize()
    host = buf.float().cpu()
    return host[:n].reshape(B, H, W, E1 + E3), host[n:], kern


def _fire_ref(t, w1, b1, w3, b3):
    """fp64 on the bf16-rounded operands."""
    x = t.double().permute(0, 3, 1, 2)
    y = torch.cat([Fn.conv2d(x, w1.double(), b1.double()), Fn.conv2d(x, w3.double(), b3.double(), padding=1)], dim=1)
    return torch.relu(y).permute(0, 2, 3, 1)


@pytest.mark.parametrize("S_", [16, 32, 48, 64])
def test_fire_expand(S_):
    E = 4 * S_
    for H, W, B in MAPS:
        g = torch.Generator().manual_seed(1000 * S_ + 10 * H + W)
        t = torch.randn(B, H, W, S_, generator=g).to(torch.bfloat16)
        w1 = (torch.randn(E, S_, 1, 1, generator=g) / np.sqrt(S_)).to(torch.bfloat16)
        w3 = (torch.randn(E, S_, 3, 3, generator=g) / np.sqrt(9 * S_)).to(torch.bfloat16)
        b1, b3 = torch.randn(E, generator=g) * 0.1, torch.randn(E, generator=g) * 0.1
        ref = _fire_ref(t, w1, b1, w3, b3)
        scale = float(ref.abs().max())
        for wide in (False, True):                              # both pixel tiles (128 / 256 per workgroup)
            y, guard, kern = _launch_fire(t, w1, b1, w3, b3, wide)
            assert kern == ("fire_expand_m256" if wide else "fire_expand_m128")
            err = (y.double() - ref).abs()
            tag = dict(S=S_, E=E, hw=(H, W), B=B, kernel=kern)
            print({**tag, "err_1x1": float(err[..., :E].max()), "err_3x3": float(err[..., E:].max()), "bound": 2.0 ** -8 * scale})
            assert bool((guard == SENTINEL).all()), tag
            assert float(err.max()) <= 2.0 ** -8 * scale, (tag, float(err.max()), scale)


def test_fire_expand_no_bias():
    """A convolution without a bias reaches the kernel as a null pointer (`ops.fire`): it stands for zeros, in either half and with the
    other half's bias applied.  S = 16, E1 = E3 = 64 on the 5 x 7 map (B = 3), both pixel tiles, the bound of `test_fire_expand`."""
    S_, E, (H, W, B) = 16, 64, MAPS[1]
    g = torch.Generator().manual_seed(160057)
    t = torch.randn(B, H, W, S_, generator=g).to(torch.bfloat16)
    w1 = (torch.randn(E, S_, 1, 1, generator=g) / np.sqrt(S_)).to(torch.bfloat16)
    w3 = (torch.randn(E, S_, 3, 3, generator=g) / np.sqrt(9 * S_)).to(torch.bfloat16)
    b1, b3 = torch.randn(E, generator=g) * 0.1, torch.randn(E, generator=g) * 0.1
    zeros = torch.zeros(E)
    for c1, c3 in ((None, b3), (b1, None)):
        ref = _fire_ref(t, w1, zeros if c1 is None else c1, w3, zeros if c3 is None else c3)
        scale = float(ref.abs().max())
        for wide in (False, True):
            y, guard, kern = _launch_fire(t, w1, c1, w3, c3, wide)
            assert kern == ("fire_expand_m256" if wide else "fire_expand_m128")
            err = (y.double() - ref).abs()
            tag = dict(b1=c1 is not None, b3=c3 is not None, kernel=kern)
            print({**tag, "err_1x1": float(err[..., :E].max()), "err_3x3": float(err[..., E:].max()), "bound": 2.0 ** -8 * scale})
            assert bool((guard == SENTINEL).all()), tag
            assert float(err.max()) <= 2.0 ** -8 * scale, (tag, float(err.max()), scale)


def test_fire_expand_exact_integers():
    """Inputs in {-2 .. 2}, weights in {-1, 0, 1}, integer biases, S = 48 on a 6 x 9 map: every partial sum is an integer below 2^24 and
    every output an integer of at most 256, exact in fp32 and in bf16 -- the output is bit-equal to the integer reference.  Every tap
    and every output channel has its own weight pattern, so a swapped tap, k-step or fragment lane cannot cancel."""
    S_, E, H, W, B = 48, 192, 6, 9, 2
    rng = np.random.default_rng(48)
    t = torch.from_numpy(rng.integers(-2, 3, (B, H, W, S_)).astype(np.float32))
    w1 = torch.from_numpy(rng.integers(-1, 2, (E, S_, 1, 1)).astype(np.float32))
    w3 = torch.from_numpy(rng.integers(-1, 2, (E, S_, 3, 3)).astype(np.float32))
    b1 = torch.from_numpy(rng.integers(-3, 4, (E,)).astype(np.float32))
    b3 = torch.from_numpy(rng.integers(-3, 4, (E,)).astype(np.float32))
    taps = w3.permute(2, 3, 0, 1).reshape(9, -1)
    assert len({tuple(r.tolist()) for r in taps}) == 9
    assert len({tuple(r.tolist()) for r in w3.reshape(E, -1)}) == E and len({tuple(r.tolist()) for r in w1.reshape(E, -1)}) == E
    assert len({tuple(r.tolist()) for r in w3.permute(1, 0, 2, 3).reshape(S_, -1)}) == S_          # ... and every input channel
    ref = _fire_ref(t, w1, b1, w3, b3)
    assert float(ref.max()) <= 256.0 and bool((ref == ref.round()).all())
    for half in (ref[..., :E], ref[..., E:]):                   # ReLU is exercised on both sides in both halves
        assert bool((half == 0).any()) and bool((half > 0).any())
    for wide in (False, True):
        y, guard, kern = _launch_fire(t.to(torch.bfloat16), w1.to(torch.bfloat16), b1, w3.to(torch.bfloat16), b3, wide)
        wrong = (y.double() != ref)
        print({"kernel": kern, "wrong": int(wrong.sum()), "of": wrong.numel()})
        assert bool((guard == SENTINEL).all())
        assert not bool(wrong.any()), (kern, int(wrong.sum()), torch.nonzero(wrong)[:8].tolist())


# ------------------------------------------------------------------------------------------------ op level: ceil-mode max pooling
@pytest.mark.parametrize("C", [8, 13])
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_ceil_maxpool(C, dtype):
    from eqxvision_amd import _lib
    tdt, code = (torch.bfloat16, _lib.BF16) if dtype == "bf16" else (torch.float32, _lib.F32)
    pool = eqv.nn.MaxPool2d(3, 2, use_ceil=True)
    for H, W in ((6, 6), (7, 10), (13, 13)):
        g = torch.Generator().manual_seed(100 * H + W + C)
        for x in (torch.randn(2, H, W, C, generator=g), -(torch.rand(2, H, W, C, generator=g) + 0.5)):      # mixed; all negative
            x = x.to(tdt)
            Ho, Wo = pool.output_size(H, W)
            ref = Fn.max_pool2d(x.float().permute(0, 3, 1, 2), 3, 2, ceil_mode=True).permute(0, 2, 3, 1)
            assert tuple(ref.shape) == (2, Ho, Wo, C)
            y = torch.full((2 * Ho * Wo * C + GUARD,), SENTINEL, dtype=tdt, device="cuda")
            xd = x.cuda()
            _lib.call("mv_maxpool2d_out_nhwc_fwd", _p(xd), _p(y), 2, H, W, C, 3, 3, 2, 2, 0, 0, Ho, Wo, code, _stream())
            torch.cuda.synchronize()
            y = y.float().cpu()
            assert bool((y[-GUARD:] == SENTINEL).all())
            assert torch.equal(y[:-GUARD].reshape(2, Ho, Wo, C), ref.contiguous()), (H, W, C, dtype)      # exact: a padded tap read as 0 shows


# ------------------------------------------------------------------------------------------------ model level
def _net(version, sd, **kw):
    with tempfile.TemporaryDirectory() as td:
        p = os.path.join(td, "w.pth")
        S.save_pth(sd, p)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return getattr(eqv.models, R.FACTORY[version])(torch_weights=p, **kw)


def _keys(B, seed=0):
    return eqv.random.split(eqv.random.PRNGKey(seed), B)


def _run(net, x, dtype="bf16", keys=None):
    with eqv.precision(dtype):
        return eqv.vmap(net, axis_name="batch")(x, key=_keys(x.shape[0]) if keys is None else keys).cpu().numpy()


def _margins(got, ref, tol):
    err = float(np.abs(got - ref).max())
    info = {"err": err, "argmax_match": float((got.argmax(-1) == ref.argmax(-1)).mean()), "max_ref": float(np.abs(ref).max())}
    print(info)
    return err <= tol, info


_CACHE = {}


def _case(version, size, B=2, seed=1):
    key = (version, size, B, seed)
    if key not in _CACHE:
        sd = R.squeezenet_state(version, seed=seed)
        x = S.synthetic_images(B, size, seed=seed)
        ref = R.forward_torch(sd, version, x)
        # the logits are averages of ReLU outputs: a dead network would pass any absolute bound
        assert float(ref.max()) >= 0.5 and float((ref > 0).mean()) > 0.5, (float(ref.max()), float((ref > 0).mean()))
        assert 1.0 <= float(np.abs(ref).max()) <= 2.0
        _CACHE[key] = (sd, x, ref, eqv.tree_inference(_net(version, sd), True))
    return _CACHE[key]


NETS = [("1_1", 64), ("1_1", 224), ("1_0", 96), ("1_0", 224)]


@pytest.mark.parametrize("version,size", NETS)
def test_bf16(version, size):
    sd, x, ref, net = _case(version, size)
    ok, info = _margins(_run(net, torch.as_tensor(x).cuda()), ref, BF16_TOL)
    assert ok, info


@pytest.mark.parametrize("version,size", NETS)
def test_fp32(version, size):
    sd, x, ref, net = _case(version, size)
    ok, info = _margins(_run(net, torch.as_tensor(x).cuda(), dtype="fp32"), ref, FP32_TOL)
    assert ok, info


@pytest.mark.parametrize("version,size", NETS)
def test_bf16_switch_off(version, size):
    from eqxvision_amd import _lib
    sd, x, ref, net = _case(version, size)
    _lib.set_flag("no_fire_expand", 1)
    try:
        off = _run(net, torch.as_tensor(x).cuda())
    finally:
        _lib.set_flag("no_fire_expand", 0)
    ok, info = _margins(off, ref, BF16_TOL)
    assert ok, info


def test_filter_jit_replay():
    sd, x, ref, net = _case("1_1", 64)
    xt = torch.as_tensor(x).cuda()
    eager = _run(net, xt)

    def body(n, im, k):
        return eqv.vmap(n, axis_name="batch")(im, key=k)

    fwd = eqv.filter_jit(body)
    with eqv.precision("bf16"):
        outs = [fwd(net, xt, _keys(2)).cpu().numpy() for _ in range(3)]          # the recording, then two replays
    for o in outs:
        assert np.array_equal(o, eager)
    ok, info = _margins(outs[-1], ref, BF16_TOL)
    assert ok, info


def test_training_mode_dropout():
    version, size = "1_1", 64
    sd, x, ref_inf, net_inf = _case(version, size)
    net = _net(version, sd)                                            # not through tree_inference: the Dropout drops
    keys = _keys(2, seed=7)
    masks = R.dropout_masks(version, size, keys)
    assert 0.4 < float(masks.mean()) < 0.6
    ref = R.forward_torch(sd, version, x, masks=masks)
    xt = torch.as_tensor(x).cuda()
    got = _run(net, xt, keys=keys)
    ok, info = _margins(got, ref, BF16_TOL)
    assert ok, info
    inf = _run(net_inf, xt, keys=keys)
    assert float(np.abs(got - inf).max()) > 10 * BF16_TOL, float(np.abs(got - inf).max())


def test_grad_refuses():
    m = eqv.models.squeezenet1_1(num_classes=3)

    @eqv.filter_value_and_grad
    def loss(model, x, y):
        out = eqv.vmap(model, axis_name="batch")(x, key=_keys(1))
        return eqv.optim.softmax_cross_entropy(out, eqv.optim.one_hot(y, 3)).mean()

    with pytest.raises(NotImplementedError, match="without a backward"):
        loss(m, torch.zeros((1, 3, 32, 32), device="cuda"), np.zeros((1,), np.int32))
