"""`-m gpu`: GoogLeNet on the MI355X -- the split pointwise kernel and the paired 3x3 kernel against fp64 convolutions on the same
bf16-rounded operands and against exact integers (strided destinations pre-filled with a sentinel, a guard behind them), ops.inception
against the literal composition, and whole networks (loaded through `torch_weights=`) against the restatement in
tests/_googlenet_ref.py.  Margins are printed (`pytest -s`)."""
import os
import tempfile
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

import eqxvision_amd as eqv
from oracle import state as S
from tests import _googlenet_ref as R
from tests._slices import SENTINEL, _check_slice, _dest, _p, _read, _stream

pytestmark = pytest.mark.gpu

BF16_TOL, FP32_TOL = 1e-2, 1e-3
MAPS_1X1 = ((1, 1, 2), (5, 7, 3), (14, 14, 1), (7, 7, 5))              # (H, W, B): one pixel; not a tile multiple; more than one tile
MAPS_3X3 = ((1, 1, 2), (5, 7, 3), (7, 7, 4), (14, 14, 1), (28, 28, 1))  # tiles that cross image borders; a map wider than a tile's halo


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from eqxvision_amd import _lib
    _lib.load()
    _lib.check_device_status()
    yield
    _lib.check_device_status()


# ------------------------------------------------------------------------------------------------ op level: mv_conv1x1_split_fwd
def _launch_split(x, w, scale, shift, n0, ld0, c0, ld1, c1):
    """x [M][C], w [N][C] bf16 -> (dst0 [M][ld0], its guard, dst1 [M][ld1] or None, its guard, the kernel's name)."""
    from eqxvision_amd import _lib
    M, C = x.shape
    N = w.shape[0]
    two = n0 < N
    assert _lib.load().mv_conv1x1_split_supported(C, N, n0, ld0, c0, ld1 if two else 0, c1 if two else 0, _lib.BF16, _lib.BF16) == 1
    d0 = _dest(M, ld0)
    d1 = _dest(M, ld1) if two else None
    xd, wd, sd, hd = x.cuda(), w.cuda(), scale.cuda(), shift.cuda()
    _lib.call("mv_conv1x1_split_fwd", _p(xd), _p(wd), _p(sd), _p(hd), _p(d0), ld0, c0, _p(d1), ld1 if two else 0, c1 if two else 0, M, C,
              N, n0, _lib.BF16, _lib.BF16, _stream())
    kern = _lib.last_kernel()
    torch.cuda.synchronize()
    y0, g0 = _read(d0, M, ld0)
    y1, g1 = _read(d1, M, ld1) if two else (None, None)
    return y0, g0, y1, g1, kern


def _split_ref(x, w, scale, shift):
    return torch.relu(x.double() @ w.double().T * scale.double() + shift.double())


@pytest.mark.parametrize("form", ["two", "one"])
def test_conv1x1_split(form):
    C, N, n0, ld0, c0, ld1, c1 = (48, 48, 16, 64, 16, 48, 0) if form == "two" else (832, 128, 128, 160, 16, 0, 0)
    for H, W, B in MAPS_1X1:
        M = B * H * W
        g = torch.Generator().manual_seed(1000 * C + 10 * H + W)
        x = torch.randn(M, C, generator=g).to(torch.bfloat16)
        w = (torch.randn(N, C, generator=g) / np.sqrt(C)).to(torch.bfloat16)
        scale, shift = torch.rand(N, generator=g) + 0.5, torch.randn(N, generator=g) * 0.1
        ref = _split_ref(x, w, scale, shift)
        bound = 2.0 ** -8 * float(ref.abs().max())
        y0, g0, y1, g1, kern = _launch_split(x, w, scale, shift, n0, ld0, c0, ld1, c1)
        tag = dict(form=form, hw=(H, W), B=B, kernel=kern)
        assert kern == ("conv1x1_split2" if form == "two" else "conv1x1_split1")
        e0 = _check_slice(y0, g0, c0, ref[:, :n0], bound, tag)
        e1 = _check_slice(y1, g1, c1, ref[:, n0:], bound, tag) if form == "two" else 0.0
        print({**tag, "err0": e0, "err1": e1, "bound": bound})


def test_conv1x1_split_exact_integers():
    """Inputs in {-2 .. 2}, weights in {-1, 0, 1}, scale 1, integer shifts, C = 80 (two k-chunks, the second a quarter full) and 23
    rows: every partial sum is an integer below 2^24 and every output an integer of at most 256, exact in fp32 and in bf16.  Every
    output channel and every input channel has its own weight pattern."""
    C, N, n0, M = 80, 176, 48, 23
    rng = np.random.default_rng(80)
    x = torch.from_numpy(rng.integers(-2, 3, (M, C)).astype(np.float32))
    w = torch.from_numpy(rng.integers(-1, 2, (N, C)).astype(np.float32))
    shift = torch.from_numpy(rng.integers(-3, 4, (N,)).astype(np.float32))
    assert len({tuple(r.tolist()) for r in w}) == N and len({tuple(r.tolist()) for r in w.T}) == C
    ref = _split_ref(x, w, torch.ones(N), shift)
    assert float(ref.max()) <= 256.0 and bool((ref == ref.round()).all()) and bool((ref == 0).any()) and bool((ref > 0).any())
    y0, g0, y1, g1, kern = _launch_split(x.to(torch.bfloat16), w.to(torch.bfloat16), torch.ones(N), shift, n0, 64, 16, 144, 16)
    _check_slice(y0, g0, 16, ref[:, :n0], 0.0, kern, exact=True)
    _check_slice(y1, g1, 16, ref[:, n0:], 0.0, kern, exact=True)


# ------------------------------------------------------------------------------------------------ op level: mv_conv3x3_pair_fwd
def _launch_pair(t, ct, w, scale, shift, ldy, cy):
    """t [B, H, W, ldt] bf16; w = (w0 [N0][S0][3][3], w1 [N1][S1][3][3]); ct / cy the slices' first channels -> (y [M][ldy], guard)."""
    from eqxvision_amd import _lib, ops
    B, H, W, ldt = t.shape
    (S0, S1), (N0, N1) = (w[0].shape[1], w[1].shape[1]), (w[0].shape[0], w[1].shape[0])
    assert _lib.load().mv_conv3x3_pair_supported(S0, S1, N0, N1, H, W, _lib.BF16, _lib.BF16) == 1
    f = [torch.from_numpy(ops.inception_fragments(v.float().numpy())).to(torch.bfloat16).cuda() for v in w]
    M = B * H * W
    y = _dest(M, ldy)
    td = t.cuda()
    sc, sh = [v.cuda() for v in scale], [v.cuda() for v in shift]
    _lib.call("mv_conv3x3_pair_fwd", _p(td), ldt, ct[0], S0, ct[1], S1, _p(f[0]), _p(sc[0]), _p(sh[0]), _p(f[1]), _p(sc[1]), _p(sh[1]),
              _p(y), ldy, cy[0], N0, cy[1], N1, B, H, W, _lib.BF16, _lib.BF16, _stream())
    assert _lib.last_kernel() == "conv3x3_pair"
    torch.cuda.synchronize()
    return _read(y, M, ldy)


def _pair_ref(t, ct, w, scale, shift):
    """fp64 on the bf16-rounded operands -> [M][N0], [M][N1]."""
    out = []
    for i in range(2):
        S_ = w[i].shape[1]
        x = t[..., ct[i]:ct[i] + S_].double().permute(0, 3, 1, 2)
        v = Fn.conv2d(x, w[i].double(), padding=1) * scale[i].double().reshape(1, -1, 1, 1) + shift[i].double().reshape(1, -1, 1, 1)
        out.append(torch.relu(v).permute(0, 2, 3, 1).reshape(-1, w[i].shape[0]))
    return out


def _check_pair(y, guard, cy, refs, bounds, tag, exact=False):
    assert bool((guard == SENTINEL).all()), tag
    own = torch.zeros(y.shape[1], dtype=torch.bool)
    errs = []
    for c, ref, bound in zip(cy, refs, bounds):
        own[c:c + ref.shape[1]] = True
        got = y[:, c:c + ref.shape[1]].double()
        if exact:
            wrong = got != ref
            assert not bool(wrong.any()), (tag, int(wrong.sum()), torch.nonzero(wrong)[:8].tolist())
        else:
            errs.append(float((got - ref).abs().max()))
            assert errs[-1] <= bound, (tag, errs[-1], bound)
    assert bool((y[:, ~own] == SENTINEL).all()), (tag, "written outside the slices")
    return errs


PAIRS = {"small": dict(ldt=64, S=(32, 16), N=(48, 16), ldy=112, cy=(16, 64)),
         "4a": dict(ldt=112, S=(96, 16), N=(208, 48), ldy=512, cy=(192, 400))}


@pytest.mark.parametrize("shape", ["small", "4a"])
def test_conv3x3_pair(shape):
    P = PAIRS[shape]
    ct = (0, P["S"][0])
    maps = MAPS_3X3 if shape == "small" else ((14, 14, 2),)
    for H, W, B in maps:
        g = torch.Generator().manual_seed(100 * H + W + P["ldy"])
        t = torch.randn(B, H, W, P["ldt"], generator=g).to(torch.bfloat16)
        w = [(torch.randn(n, s, 3, 3, generator=g) / np.sqrt(9 * s)).to(torch.bfloat16) for n, s in zip(P["N"], P["S"])]
        scale = [torch.rand(n, generator=g) + 0.5 for n in P["N"]]
        shift = [torch.randn(n, generator=g) * 0.1 for n in P["N"]]
        refs = _pair_ref(t, ct, w, scale, shift)
        bounds = [2.0 ** -8 * float(r.abs().max()) for r in refs]
        y, guard = _launch_pair(t, ct, w, scale, shift, P["ldy"], P["cy"])
        tag = dict(shape=shape, hw=(H, W), B=B)
        errs = _check_pair(y, guard, P["cy"], refs, bounds, tag)
        print({**tag, "err": errs, "bound": bounds})


def test_conv3x3_pair_exact_integers():
    """Inputs in {-2 .. 2}, weights in {-1, 0, 1}, scale 1, integer shifts, slices of 48 and 16 channels to 80 and 48 outputs (an odd
    tile count and a half tile) on a 6 x 9 map, 3 images: bit-equal to the integer reference.  Every tap, every output channel and
    every input channel has its own weight pattern, so a swapped tap, k-step or fragment lane cannot cancel."""
    S_, N, H, W, B = (48, 16), (80, 48), 6, 9, 3
    rng = np.random.default_rng(3348)
    t = torch.from_numpy(rng.integers(-2, 3, (B, H, W, 80)).astype(np.float32))
    w = [torch.from_numpy(rng.integers(-1, 2, (n, s, 3, 3)).astype(np.float32)) for n, s in zip(N, S_)]
    for v in w:
        n, s = v.shape[:2]
        assert len({tuple(r.tolist()) for r in v.permute(2, 3, 0, 1).reshape(9, -1)}) == 9
        assert len({tuple(r.tolist()) for r in v.reshape(n, -1)}) == n
        assert len({tuple(r.tolist()) for r in v.permute(1, 0, 2, 3).reshape(s, -1)}) == s
    scale = [torch.ones(n) for n in N]
    shift = [torch.from_numpy(rng.integers(-3, 4, (n,)).astype(np.float32)) for n in N]
    ct, cy = (16, 64), (96, 16)                                        # the second slice is written BEFORE the first in y
    refs = _pair_ref(t, ct, w, scale, shift)
    for r in refs:
        assert float(r.max()) <= 256.0 and bool((r == r.round()).all()) and bool((r == 0).any()) and bool((r > 0).any())
    y, guard = _launch_pair(t.to(torch.bfloat16), ct, [v.to(torch.bfloat16) for v in w], scale, shift, 192, cy)
    _check_pair(y, guard, cy, refs, (0.0, 0.0), "exact", exact=True)


# ------------------------------------------------------------------------------------------------ ops.inception
def test_inception_against_composition():
    """One small module with c5r = 24 (the padded reduce slice) at 7 x 7, B = 3: 4 launches, no concatenation, and the literal
    composition's numbers to the bound of the op-level tests (both round every intermediate to bf16)."""
    from eqxvision_amd import _lib, ops
    from eqxvision_amd._act import Act
    from eqxvision_amd.models.classification.googlenet import _Inception
    mod = eqv.tree_inference(eqv.utils.randomize_batchnorm(_Inception(64, 32, 48, 80, 24, 16, 32, key=eqv.random.PRNGKey(5))), True)
    x = Act(torch.randn(3, 7, 7, 64, generator=torch.Generator().manual_seed(5)).to(torch.bfloat16).cuda(), "map", True)
    with eqv.precision("bf16"):
        rec = []
        old = _lib.set_recording(rec)
        try:
            fused = ops.inception(x, mod)
        finally:
            _lib.set_recording(old)
        names = [r[2] for r in rec]
        assert names == ["mv_conv1x1_split_fwd", "mv_maxpool2d_nhwc_fwd", "mv_conv1x1_split_fwd", "mv_conv3x3_pair_fwd"], names
        assert _lib.last_kernel() == "conv3x3_pair"
        _lib.set_flag("no_inception_fused", 1)
        try:
            rec = []
            old = _lib.set_recording(rec)
            try:
                lit = ops.inception(x, mod)
            finally:
                _lib.set_recording(old)
        finally:
            _lib.set_flag("no_inception_fused", 0)
        names = [r[2] for r in rec]
        assert names.count("mv_conv2d_nhwc_fwd") == 6 and names.count("mv_copy_rows") == 4 and "mv_conv3x3_pair_fwd" not in names, names
    torch.cuda.synchronize()
    a, b = fused.t.float().cpu(), lit.t.float().cpu()
    assert tuple(a.shape) == (3, 7, 7, 32 + 80 + 16 + 32)
    err, scale = float((a - b).abs().max()), float(b.abs().max())
    print({"err": err, "bound": 2.0 ** -7 * scale})
    # two bf16 roundings (the reduce map, the output) on each side: twice the one-rounding bound of the op-level tests
    assert err <= 2.0 ** -7 * scale and scale > 0.5


# ------------------------------------------------------------------------------------------------ model level
def _net(sd, **kw):
    with tempfile.TemporaryDirectory() as td:
        p = os.path.join(td, "w.pth")
        S.save_pth(sd, p)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return eqv.models.googlenet(torch_weights=p, **kw)


def _keys(B, seed=0):
    return eqv.random.split(eqv.random.PRNGKey(seed), B)


def _run(net, x, dtype="bf16", keys=None):
    with eqv.precision(dtype):
        out = eqv.vmap(net, axis_name="batch")(x, key=_keys(x.shape[0]) if keys is None else keys)
    assert isinstance(out, tuple) and len(out) == 3
    return tuple(o.cpu().numpy() for o in out)


def _margins(got, ref, tol):
    ok, info = True, {}
    for name, g, r in zip(("logits", "aux2", "aux1"), got, ref):
        err = float(np.abs(g - r).max())
        info[name] = {"err": err, "argmax_match": float((g.argmax(-1) == r.argmax(-1)).mean()), "max_ref": float(np.abs(r).max())}
        ok = ok and g.shape == r.shape and err <= tol
    print(info)
    return ok, info


_CACHE = {}


def _case(size, B, seed=1):
    key = (size, B, seed)
    if key not in _CACHE:
        if "sd" not in _CACHE:
            _CACHE["sd"] = R.googlenet_state(seed=seed)
            _CACHE["net"] = eqv.tree_inference(_net(_CACHE["sd"], aux_logits=True), True)
        x = S.synthetic_images(B, size, seed=seed)
        ref = R.forward_torch(_CACHE["sd"], x)
        for r in ref:                                                  # a dead network would pass any absolute bound
            assert 1.0 <= float(np.abs(r).max()) <= 3.0 and 0.3 < float((r > 0).mean()) < 0.7
        _CACHE[key] = (x, ref)
    return _CACHE["sd"], _CACHE[key][0], _CACHE[key][1], _CACHE["net"]


# 75: the issue's case (pool 1 grows: 38 -> 19; modules on 9 / 4 / 2 maps, aux pools 4 to 4); 80: EVERY ceil pool grows its output
# (40 -> 20 -> 10 -> 5 -> 3), the modules run on 10 x 10, 5 x 5 and 3 x 3 maps and the auxiliary heads pool 5 to 4
NETS = [(224, 2), (75, 3), (80, 3)]


@pytest.mark.parametrize("size,B", NETS)
def test_bf16(size, B):
    sd, x, ref, net = _case(size, B)
    ok, info = _margins(_run(net, torch.as_tensor(x).cuda()), ref, BF16_TOL)
    assert ok, info


@pytest.mark.parametrize("size,B", NETS)
def test_fp32(size, B):
    sd, x, ref, net = _case(size, B)
    ok, info = _margins(_run(net, torch.as_tensor(x).cuda(), dtype="fp32"), ref, FP32_TOL)
    assert ok, info


def test_bf16_switch_off():
    from eqxvision_amd import _lib
    sd, x, ref, net = _case(224, 2)
    _lib.set_flag("no_inception_fused", 1)
    try:
        off = _run(net, torch.as_tensor(x).cuda())
    finally:
        _lib.set_flag("no_inception_fused", 0)
    ok, info = _margins(off, ref, BF16_TOL)
    assert ok, info


def test_filter_jit_lanes():
    sd, x, ref, net = _case(224, 2)
    xt = torch.as_tensor(x).cuda()
    eager = _run(net, xt)

    def body(n, im, k):
        return eqv.vmap(n, axis_name="batch")(im, key=k)

    fwd = eqv.filter_jit(body, lanes=2)
    with eqv.precision("bf16"):
        outs = [tuple(o.cpu().numpy() for o in fwd(net, xt, _keys(2))) for _ in range(3)]      # the recording, then two replays
    for o in outs:
        assert len(o) == 3
        ok, info = _margins(o, ref, BF16_TOL)
        assert ok, info
    for a, b in zip(outs[-1], outs[0]):
        assert np.array_equal(a, b)
    for a, b in zip(outs[-1], eager):                                  # a lane is one image here: the kernels' tiles differ, not the sums' order
        assert float(np.abs(a - b).max()) <= BF16_TOL


def test_single_output_without_aux():
    sd, x, ref, net = _case(75, 3)
    plain = eqv.tree_inference(_net(sd), True)
    assert plain.aux_logits is False
    with eqv.precision("bf16"):
        out = eqv.vmap(plain, axis_name="batch")(torch.as_tensor(x).cuda(), key=_keys(3))
    assert isinstance(out, torch.Tensor) and tuple(out.shape) == (3, 1000)
    assert float(np.abs(out.cpu().numpy() - ref[0]).max()) <= BF16_TOL


def test_training_mode_forward():
    """Batch-statistics BatchNorm and the three Dropouts live under fixed keys at 75 x 75, B = 4: the restatement with the keep masks
    of the reference's key schedule; the running statistics move.  Measured on one MI355X: logits 3.7e-3, aux2 4.6e-3, aux1 5.8e-3
    of the 1e-2 bound.  With the inference checkpoint (AUX_SCALE) the dropped-out aux logits reach 3.2 / 3.5 and their errors 8.3e-3 /
    1.04e-2: the training checkpoint keeps them around 2, which the absolute bound is meant for (tests/_googlenet_ref.py)."""
    sd = R.googlenet_state(seed=1, aux_scale=R.AUX_SCALE_TRAIN)      # max |logit| around 2 with the Dropouts live (see the constant)
    net = _net(sd, aux_logits=True)                                    # not through tree_inference
    x = S.synthetic_images(4, 75, seed=1)
    keys = _keys(4, seed=7)
    masks = R.dropout_masks(keys)
    assert 0.7 < float(masks["main"].mean()) < 0.9 and 0.2 < float(masks["aux1"].mean()) < 0.4
    new_running = {}
    ref = R.forward_torch(sd, x, train=True, masks=masks, new_running=new_running)
    got = _run(net, torch.as_tensor(x).cuda(), keys=keys)
    for r in ref:
        assert 1.0 <= float(np.abs(r).max()) <= 3.0
    ok, info = _margins(got, ref, BF16_TOL)
    assert ok, info
    nodrop = R.forward_torch(sd, x, train=True)
    assert float(np.abs(nodrop[0] - ref[0]).max()) > 10 * BF16_TOL     # the masks matter
    for name in ("conv1.bn", "inception4b.branch3.1.bn", "aux2.conv.bn"):
        node = net
        for part in name.split("."):
            node = node.layers[int(part)] if part.isdigit() else getattr(node, part)
        mean, var = node.state_index.value
        rm, rv = new_running[name]
        old = np.asarray(sd[name + ".running_mean"])
        assert float(np.abs(np.asarray(mean) - old).max()) > 1e-5
        np.testing.assert_allclose(np.asarray(mean), rm, atol=2e-3)
        np.testing.assert_allclose(np.asarray(var), rv, rtol=2e-2, atol=1e-3)


def test_grad_refuses():
    m = eqv.models.googlenet(num_classes=3)

    @eqv.filter_value_and_grad
    def loss(model, x, y):
        out = eqv.vmap(model, axis_name="batch")(x, key=_keys(1))
        return eqv.optim.softmax_cross_entropy(out, eqv.optim.one_hot(y, 3)).mean()

    with pytest.raises(NotImplementedError, match="without a backward"):
        loss(m, torch.zeros((1, 3, 32, 32), device="cuda"), np.zeros((1,), np.int32))
