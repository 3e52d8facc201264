"""`-m gpu`: DenseNet on the MI355X -- the pre-activated pointwise kernel (bottleneck and transition forms) and the 3x3 slice kernel
against fp64 on the same bf16 operands and against exact integers (strided destinations pre-filled with a sentinel, a guard behind
them, NaN in the part of the source rows that must not be read), ops.dense_block + ops.dense_transition against the literal
composition, and whole networks (loaded through `torch_weights=`) against the restatement in tests/_densenet_ref.py.  Margins are
printed (`pytest -s`)."""
import os
import tempfile
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

import eqxvision_amd as eqv
from oracle import state as S
from tests import _densenet_ref as R
from tests._slices import _check_slice, _dest, _p, _read, _stream

pytestmark = pytest.mark.gpu

BF16_TOL, FP32_TOL = 1e-2, 1e-3
MAPS_1X1 = ((1, 1, 2), (5, 7, 3), (14, 14, 1), (7, 7, 5))              # (H, W, B): one pixel; not a tile multiple; more than one tile
MAPS_POOL = ((4, 4, 3), (5, 7, 2), (2, 2, 1), (15, 14, 2))              # 5 x 7 -> 2 x 3 and 15 x 14 -> 7 x 7: an odd row / column is dropped
MAPS_3X3 = ((1, 1, 2), (5, 7, 3), (7, 7, 4), (14, 14, 1), (28, 28, 1))  # tests/test_googlenet_gpu.py


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from eqxvision_amd import _lib
    _lib.load()
    _lib.check_device_status()
    yield
    _lib.check_device_status()


# ------------------------------------------------------------------------------------------------ op level: mv_preact_conv1x1_fwd
def _launch_preact(x, C, s1, h1, w, s2, h2, ldy, cy, pool):
    """x [B, H, W, ldx] bf16 (channels >= C may hold anything), w [N][C] bf16 -> (y [Mo][ldy], its guard, the kernel's name)."""
    from eqxvision_amd import _lib
    B, H, W, ldx = x.shape
    N = w.shape[0]
    assert _lib.load().mv_preact_conv1x1_supported(C, N, ldx, ldy, cy, pool, _lib.BF16, _lib.BF16) == 1
    Mo = B * (H // pool) * (W // pool)
    y = _dest(Mo, ldy)
    xd, wd, s1d, h1d = x.cuda(), w.cuda(), s1.cuda(), h1.cuda()
    s2d, h2d = (None, None) if s2 is None else (s2.cuda(), h2.cuda())
    _lib.call("mv_preact_conv1x1_fwd", _p(xd), ldx, _p(s1d), _p(h1d), _p(wd), _p(s2d), _p(h2d), _p(y), ldy, cy, B, H, W, C, N, pool,
              _lib.BF16, _lib.BF16, _stream())
    kern = _lib.last_kernel()
    torch.cuda.synchronize()
    return _read(y, Mo, ldy) + (kern,)


def _preact_ref(x, C, s1, h1, w, s2, h2, pool):
    """fp64 on the same bf16 operands, `a` rounded to bf16 -> ([Mo][N], a [Mo][C] as fp64)."""
    B, H, W, _ = x.shape
    r = torch.relu(x[..., :C].double() * s1.double() + h1.double())
    if pool == 2:
        Ho, Wo = H // 2, W // 2
        r = r[:, :2 * Ho, :2 * Wo].reshape(B, Ho, 2, Wo, 2, C).mean((2, 4))
    a = r.reshape(-1, C).to(torch.bfloat16).double()
    v = a @ w.double().T
    if s2 is not None:
        v = torch.relu(v * s2.double() + h2.double())
    return v, a


def _preact_case(C, N, ldx, H, W, B, pool, post, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, H, W, ldx, generator=g).to(torch.bfloat16)
    x[..., C:] = float("nan")                                          # memory a later layer has not written yet
    w = (torch.randn(N, C, generator=g) / np.sqrt(C)).to(torch.bfloat16)
    s1 = torch.rand(C, generator=g) + 0.5
    h1 = torch.randn(C, generator=g) * 0.5                             # non-zero, both signs: relu(0 * s + h) is not zero
    assert bool((h1 > 0.05).any()) and bool((h1 < -0.05).any())
    s2, h2 = (torch.rand(N, generator=g) + 0.5, torch.randn(N, generator=g) * 0.1) if post else (None, None)
    return x, w, s1, h1, s2, h2


@pytest.mark.parametrize("shape", [(80, 128, 112), (208, 192, 384)])
def test_preact_bottleneck(shape):
    """p = 1, BatchNorm 2 + ReLU behind the product, dense y.  C = 80: two chunks, the second a quarter full; channels [C, ldx) of
    x are NaN.  Bound 2^-7 max|ref|: twice the one-rounding bound of the other op tests, because an fma can flip the rounding of `a`
    by one ulp."""
    C, N, ldx = shape
    for H, W, B in MAPS_1X1:
        x, w, s1, h1, s2, h2 = _preact_case(C, N, ldx, H, W, B, 1, True, 1000 * C + 10 * H + W)
        ref, _ = _preact_ref(x, C, s1, h1, w, s2, h2, 1)
        bound = 2.0 ** -7 * float(ref.abs().max())
        y, guard, kern = _launch_preact(x, C, s1, h1, w, s2, h2, N, 0, 1)
        assert kern == "preact1x1_relu"
        tag = dict(C=C, hw=(H, W), B=B, kernel=kern)
        err = _check_slice(y, guard, 0, ref, bound, tag)
        print({**tag, "err": err, "bound": bound})


def test_preact_transition():
    """p = 2, the identity behind the product, into channels [16, 64) of rows of 112; the reference holds negative values."""
    C, N, ldy, cy = 96, 48, 112, 16
    for H, W, B in MAPS_POOL:
        x, w, s1, h1, _, _ = _preact_case(C, N, C + 32, H, W, B, 2, False, 77 * H + W)
        ref, _ = _preact_ref(x, C, s1, h1, w, None, None, 2)
        assert ref.shape[0] == B * (H // 2) * (W // 2) and float(ref.min()) < -0.1 < 0.1 < float(ref.max())
        bound = 2.0 ** -7 * float(ref.abs().max())
        y, guard, kern = _launch_preact(x, C, s1, h1, w, None, None, ldy, cy, 2)
        assert kern == "preact1x1_pool2"
        tag = dict(hw=(H, W), B=B, kernel=kern)
        err = _check_slice(y, guard, cy, ref, bound, tag)
        neg = ref < -0.1
        assert float((y[:, cy:cy + N].double() - ref)[neg].abs().max()) <= bound and bool((y[:, cy:cy + N][neg] < 0).all())
        print({**tag, "err": err, "bound": bound})


@pytest.mark.parametrize("pool", [1, 2])
def test_preact_exact_integers(pool):
    """x in {-2 .. 2}, s1 in {1, 2}, integer h1, w in {-1, 0, 1}, integer h2 (bottleneck form) or the identity (transition form);
    C = 80 (two chunks, the second a quarter full): every `a` is an integer (a quarter-integer below 8 under p = 2) and every output
    a (quarter-)integer of magnitude below 512, all exact in bf16 -- asserted -- so the result is bit-equal.  Every output channel
    and every input channel has its own weight pattern."""
    C, N, ldx, H, W, B = 80, 176, 112, 5, 6, 2
    rng = np.random.default_rng(80 + pool)
    x = torch.from_numpy(rng.integers(-2, 3, (B, H, W, ldx)).astype(np.float32))
    x[..., C:] = float("nan")
    # few non-zero weights per row keep |v| small enough for quarter-integers to stay exact in bf16 (8 bits: |v| < 64 at 1/4 steps)
    w = torch.from_numpy((rng.integers(-1, 2, (N, C)) * (rng.random((N, C)) < 0.15)).astype(np.float32))
    assert len({tuple(r.tolist()) for r in w}) == N and len({tuple(r.tolist()) for r in w.T}) == C
    s1 = torch.from_numpy(rng.integers(1, 3, (C,)).astype(np.float32))
    h1 = torch.from_numpy(rng.integers(-2, 3, (C,)).astype(np.float32))
    post = pool == 1
    s2 = torch.ones(N) if post else None
    h2 = torch.from_numpy(rng.integers(-3, 4, (N,)).astype(np.float32)) if post else None
    xb, wb = x.to(torch.bfloat16), w.to(torch.bfloat16)
    ref, a = _preact_ref(xb, C, s1, h1, wb, s2, h2, pool)
    r = torch.relu(xb[..., :C].double() * s1.double() + h1.double())
    if pool == 2:
        r = r[:, :4, :6].reshape(B, 2, 2, 3, 2, C).mean((2, 4))
    assert bool((a == r.reshape(-1, C)).all()) and bool((a * pool * pool == (a * pool * pool).round()).all())      # `a` exact in bf16
    assert bool((ref == ref.to(torch.bfloat16).double()).all()) and float(ref.abs().max()) < 512.0               # the outputs too
    assert bool((ref > 0).any()) and (post or bool((ref < 0).any())) and (pool == 1 or bool((ref != ref.round()).any()))
    ldy, cy = (N, 0) if post else (N + 32, 16)
    y, guard, kern = _launch_preact(xb, C, s1, h1, wb, s2, h2, ldy, cy, pool)
    _check_slice(y, guard, cy, ref, 0.0, kern, exact=True)


# ------------------------------------------------------------------------------------------------ op level: mv_conv3x3_slice_fwd
def _launch_slice(t, S_, w, ldy, cy, flag=None):
    from eqxvision_amd import _lib, ops
    B, H, W, ldt = t.shape
    N = w.shape[0]
    assert _lib.load().mv_conv3x3_slice_supported(S_, N, H, W, _lib.BF16, _lib.BF16) == 1
    f = torch.from_numpy(ops.inception_fragments(w.float().numpy())).to(torch.bfloat16).cuda()
    M = B * H * W
    y = _dest(M, ldy)
    td = t.cuda()
    if flag:
        _lib.set_flag(flag, 1)
    try:
        _lib.call("mv_conv3x3_slice_fwd", _p(td), ldt, S_, _p(f), _p(y), ldy, cy, N, B, H, W, _lib.BF16, _lib.BF16, _stream())
    finally:
        if flag:
            _lib.set_flag(flag, 0)
    kern = _lib.last_kernel()
    torch.cuda.synchronize()
    return _read(y, M, ldy) + (kern,)


def _slice_ref(t, S_, w):
    x = t[..., :S_].double().permute(0, 3, 1, 2)
    return Fn.conv2d(x, w.double(), padding=1).permute(0, 2, 3, 1).reshape(-1, w.shape[0])


@pytest.mark.parametrize("S_,N", [(128, 32), (192, 48)])
@pytest.mark.parametrize("pad", [0, 16])
def test_conv3x3_slice(S_, N, pad):
    """Into channels [48, 48 + N) of rows of 96, from rows of S and of S + 16 (the extra channels NaN); both pixel tiles.  N = 48:
    the upper half of the second tile is never stored.  No ReLU: the negative half of the reference must come through."""
    ldy, cy = 96, 48
    for H, W, B in MAPS_3X3:
        g = torch.Generator().manual_seed(100 * H + W + S_ + pad)
        t = torch.randn(B, H, W, S_ + pad, generator=g).to(torch.bfloat16)
        t[..., S_:] = float("nan")
        w = (torch.randn(N, S_, 3, 3, generator=g) / np.sqrt(9 * S_)).to(torch.bfloat16)
        ref = _slice_ref(t, S_, w)
        assert float(ref.min()) < -0.1 < 0.1 < float(ref.max())
        bound = 2.0 ** -8 * float(ref.abs().max())
        for flag, name in ((None, "conv3x3_slice_m64"), ("dense3x3_m128", "conv3x3_slice_m128")):
            y, guard, kern = _launch_slice(t, S_, w, ldy, cy, flag)
            assert kern == name
            tag = dict(S=S_, N=N, ldt=S_ + pad, hw=(H, W), B=B, kernel=kern)
            err = _check_slice(y, guard, cy, ref, bound, tag)
            neg = ref < -0.1
            assert bool((y[:, cy:cy + N][neg] < 0).all()), tag
            print({**tag, "err": err, "bound": bound})


def test_conv3x3_slice_exact_integers():
    """Inputs in {-2 .. 2}, weights in {-1, 0, 1}, 128 channels to 48 outputs on a 6 x 9 map, 3 images: bit-equal to the integer
    reference, negatives included.  Every tap, every output channel and every input channel has its own weight pattern."""
    S_, N, H, W, B = 128, 48, 6, 9, 3
    rng = np.random.default_rng(12848)
    t = torch.from_numpy(rng.integers(-2, 3, (B, H, W, S_)).astype(np.float32))
    w = torch.from_numpy((rng.integers(-1, 2, (N, S_, 3, 3)) * (rng.random((N, S_, 3, 3)) < 0.1)).astype(np.float32))
    assert len({tuple(r.tolist()) for r in w.permute(2, 3, 0, 1).reshape(9, -1)}) == 9
    assert len({tuple(r.tolist()) for r in w.reshape(N, -1)}) == N
    assert len({tuple(r.tolist()) for r in w.permute(1, 0, 2, 3).reshape(S_, -1)}) == S_
    ref = _slice_ref(t, S_, w)
    assert float(ref.abs().max()) <= 256.0 and bool((ref == ref.round()).all()) and bool((ref < 0).any()) and bool((ref > 0).any())
    for flag in ("dense3x3_m64", "dense3x3_m128"):
        y, guard, kern = _launch_slice(t.to(torch.bfloat16), S_, w.to(torch.bfloat16), 96, 48, flag)
        _check_slice(y, guard, 48, ref, 0.0, kern, exact=True)


# ------------------------------------------------------------------------------------------------ ops.dense_block / ops.dense_transition
@pytest.mark.parametrize("H,W,B", [(7, 7, 3), (5, 7, 2)])
def test_block_and_transition_against_composition(H, W, B):
    """_DenseBlock(3, 48, bn_size 2, growth 16) + _Transition(96, 48): 1 + 2 * 3 + 1 launches, and the literal composition's numbers
    to 2^-7 max|composition| (both sides round the same three intermediates per layer to bf16)."""
    from eqxvision_amd import _lib, ops
    from eqxvision_amd._act import Act
    from eqxvision_amd.models.classification.densenet import _DenseBlock, _Transition
    blk = eqv.tree_inference(eqv.utils.randomize_batchnorm(_DenseBlock(3, 48, 2, 16, 0.0, key=eqv.random.PRNGKey(5))), True)
    tr = eqv.tree_inference(eqv.utils.randomize_batchnorm(_Transition(96, 48, key=eqv.random.PRNGKey(6)), seed=2), True)
    x = Act(torch.randn(B, H, W, 48, generator=torch.Generator().manual_seed(5)).to(torch.bfloat16).cuda(), "map", True)

    def both():
        rec = []
        old = _lib.set_recording(rec)
        try:
            y = ops.dense_block(x, blk)
            z = ops.dense_transition(y, tr)
        finally:
            _lib.set_recording(old)
        return y, z, [r[2] for r in rec]
    with eqv.precision("bf16"):
        yf, zf, names = both()
        assert names == ["mv_copy_rows"] + ["mv_preact_conv1x1_fwd", "mv_conv3x3_slice_fwd"] * 3 + ["mv_preact_conv1x1_fwd"], names
        _lib.set_flag("no_dense_fused", 1)
        try:
            yl, zl, names = both()
        finally:
            _lib.set_flag("no_dense_fused", 0)
        assert "mv_preact_conv1x1_fwd" not in names and names.count("mv_conv2d_nhwc_fwd") == 7 and names[-1] == "mv_avgpool2d_nhwc_fwd"
    torch.cuda.synchronize()
    for a, b, shape in ((yf, yl, (B, H, W, 96)), (zf, zl, (B, H // 2, W // 2, 48))):
        a, b = a.t.float().cpu(), b.t.float().cpu()
        assert tuple(a.shape) == tuple(b.shape) == shape
        err, scale = float((a - b).abs().max()), float(b.abs().max())
        print({"shape": shape, "err": err, "bound": 2.0 ** -7 * scale})
        assert err <= 2.0 ** -7 * scale and scale > 0.5


# ------------------------------------------------------------------------------------------------ model level
def _net(variant, sd, **kw):
    with tempfile.TemporaryDirectory() as td:
        p = os.path.join(td, "w.pth")
        S.save_pth(sd, p)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return getattr(eqv.models, variant)(torch_weights=p, **kw)


def _keys(B, seed=0):
    return eqv.random.split(eqv.random.PRNGKey(seed), B)


def _run(net, x, dtype="bf16", keys=None):
    with eqv.precision(dtype):
        out = eqv.vmap(net, axis_name="batch")(x, key=_keys(x.shape[0]) if keys is None else keys)
    return out.cpu().numpy()


def _margin(got, ref, tol, tag):
    err = float(np.abs(got - ref).max())
    info = {"case": tag, "err": err, "tol": tol, "argmax_match": float((got.argmax(-1) == ref.argmax(-1)).mean()),
            "max_ref": float(np.abs(ref).max())}
    print(info)
    return got.shape == ref.shape and err <= tol, info


_CACHE = {}


def _case(variant, size, B, seed=1):
    if variant not in _CACHE:
        sd = R.densenet_state(variant, seed=seed)
        _CACHE[variant] = (sd, eqv.tree_inference(_net(variant, sd), True))
    sd, net = _CACHE[variant]
    key = (variant, size, B)
    if key not in _CACHE:
        ref = R.logits(sd, R.case_features(variant, seed, size, B))
        # a dead network would pass any absolute bound
        assert 1.0 <= float(np.abs(ref).max()) <= 3.0 and 0.3 <= float((ref > 0).mean()) <= 0.7
        _CACHE[key] = (S.synthetic_images(B, size, seed=seed), ref)
    return sd, _CACHE[key][0], _CACHE[key][1], net


# densenet121 at 80: the maps are 20 / 10 / 5 / 2 -- the third transition pools 5 -> 2
NETS = [(v, size, B) for v in R.VARIANTS for size, B in R.CASES[v]]


@pytest.mark.parametrize("variant,size,B", NETS)
def test_bf16(variant, size, B):
    sd, x, ref, net = _case(variant, size, B)
    ok, info = _margin(_run(net, torch.as_tensor(x).cuda()), ref, BF16_TOL, (variant, size, B))
    assert ok, info


@pytest.mark.parametrize("variant,size,B", NETS)
def test_fp32(variant, size, B):
    sd, x, ref, net = _case(variant, size, B)
    ok, info = _margin(_run(net, torch.as_tensor(x).cuda(), dtype="fp32"), ref, FP32_TOL, (variant, size, B))
    assert ok, info


def test_bf16_switch_off():
    from eqxvision_amd import _lib
    sd, x, ref, net = _case("densenet121", 224, 2)
    _lib.set_flag("no_dense_fused", 1)
    try:
        off = _run(net, torch.as_tensor(x).cuda())
    finally:
        _lib.set_flag("no_dense_fused", 0)
    ok, info = _margin(off, ref, BF16_TOL, "composition 121 / 224")
    assert ok, info


def test_filter_jit_lanes():
    sd, x, ref, net = _case("densenet121", 224, 2)
    xt = torch.as_tensor(x).cuda()
    eager = _run(net, xt)

    def body(n, im, k):
        return eqv.vmap(n, axis_name="batch")(im, key=k)

    fwd = eqv.filter_jit(body, lanes=2)
    with eqv.precision("bf16"):
        outs = [fwd(net, xt, _keys(2)).cpu().numpy() for _ in range(3)]          # the recording, then two replays
    for o in outs:
        ok, info = _margin(o, ref, BF16_TOL, "lanes")
        assert ok, info
    assert np.array_equal(outs[-1], outs[0])
    assert float(np.abs(outs[-1] - eager).max()) <= BF16_TOL           # a lane is one image here: the tiles differ, not the sums' order


def test_training_mode_forward():
    """densenet121, 64 x 64, B = 4, drop_rate 0, BatchNorm on batch statistics (the composition) against the restatement's training
    branch; the running statistics move."""
    variant = "densenet121"
    sd = R.densenet_state(variant, seed=1)
    net = _net(variant, sd)                                            # not through tree_inference
    x = S.synthetic_images(4, 64, seed=1)
    new_running = {}
    ref = R.forward_torch(sd, variant, x, train=True, new_running=new_running)
    assert 1.0 <= float(np.abs(ref).max()) <= 3.0
    ok, info = _margin(_run(net, torch.as_tensor(x).cuda()), ref, BF16_TOL, "training 121 / 64")
    assert ok, info
    L = net.features.layers
    for node, name in ((L[1], "features.norm0"), (L[6].layers[4].norm2, "features.denseblock2.denselayer5.norm2"),
                       (L[7].layers.layers[0], "features.transition2.norm"), (L[-3], "features.norm5")):
        mean, var = node.state_index.value
        rm, rv = new_running[name]
        old = np.asarray(sd[name + ".running_mean"])
        assert float(np.abs(np.asarray(mean) - old).max()) > 1e-5
        np.testing.assert_allclose(np.asarray(mean), rm, atol=2e-3)
        np.testing.assert_allclose(np.asarray(var), rv, rtol=2e-2, atol=1e-3)


def test_grad_refuses():
    m = eqv.models.densenet121(num_classes=3)

    @eqv.filter_value_and_grad
    def loss(model, x, y):
        out = eqv.vmap(model, axis_name="batch")(x, key=_keys(1))
        return eqv.optim.softmax_cross_entropy(out, eqv.optim.one_hot(y, 3)).mean()

    with pytest.raises(NotImplementedError, match="without a backward"):
        loss(m, torch.zeros((1, 3, 32, 32), device="cuda"), np.zeros((1,), np.int32))
