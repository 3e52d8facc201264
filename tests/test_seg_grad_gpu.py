"""`-m gpu`: the training step of fcn / deeplabv3 / lraspp_mobilenet_v3_large on the MI355X.

Kernel level: mv_resize_bilinear_bwd_nhwc_f32 against torch.autograd -- bit-equal where the arithmetic is exact (dyadic ratios,
integer gradients), within a per-element bound derived from the index arithmetic otherwise -- and against the project's own forward
kernel through <resize(x), dy> == <x, resize_bwd(dy)>; mv_softmax_xent_map_f32 against F.cross_entropy in float64.  Every kernel is
run twice on the same input: the bits must not change.
Model level: every parameter gradient of mean(xent(out)) + 0.4 mean(xent(aux)) against torch.autograd on tests/_seg_grad_ref.py
under grad_parity_case's criterion, and two Adam steps of each model fresh from its factory (training mode).
Figures are printed (`pytest -s`)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import eqxvision_amd as eqv
from eqxvision_amd import _lib
from tests import _seg_grad_ref as R
from tests._cases import TOL_F32, _cmp
from tests._model_cases import _keys, _load
from tests._slices import GUARD, SENTINEL, _p, _stream

pytestmark = pytest.mark.gpu
U = R.U


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    _lib.load()
    _lib.check_device_status()
    yield
    _lib.check_device_status()


def _ids(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


# ------------------------------------------------------------------------------------------------ 1. resize backward
def _resize_bwd(dy_nchw: np.ndarray, shape, size, nchw: bool) -> np.ndarray:
    """dx [B, h, w, C] from the kernel, run twice into sentinel-filled buffers with a guard behind them; the two runs bit-equal."""
    B, h, w, C = shape
    H, W = size
    dy = torch.from_numpy(np.ascontiguousarray(dy_nchw if nchw else dy_nchw.transpose(0, 2, 3, 1))).cuda()
    n = B * h * w * C
    runs = []
    for _ in range(2):
        dx = torch.full((n + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
        _lib.call("mv_resize_bilinear_bwd_nhwc_f32", _p(dy), _p(dx), B, h, w, C, H, W, int(nchw), _stream())
        torch.cuda.synchronize()
        runs.append(dx.cpu())
    assert torch.equal(runs[0].view(torch.int32), runs[1].view(torch.int32)), "two runs differ"
    assert bool((runs[0][n:] == SENTINEL).all()), "written past the end of dx"
    got = runs[0][:n].numpy().reshape(B, h, w, C)
    assert np.isfinite(got).all()
    return got


def _torch_resize_bwd(dy_nchw: np.ndarray, shape, size) -> np.ndarray:
    B, h, w, C = shape
    x = torch.zeros(B, C, h, w, requires_grad=True)
    R.resize(x, size).backward(torch.from_numpy(dy_nchw))
    return x.grad.numpy().transpose(0, 2, 3, 1)


@pytest.mark.parametrize("nchw", [True, False], ids=["dy_nchw", "dy_nhwc"])
@pytest.mark.parametrize("shape,size", R.RESIZE_EXACT, ids=_ids)
def test_resize_bwd_exact(shape, size, nchw):
    """Weights are multiples of 1/16 (or 1/4, or 1), dy integers in [-8, 8]: every product and partial sum is exact in fp32, so the
    result equals torch's in any summation order."""
    B, h, w, C = shape
    dy = np.random.Generator(np.random.PCG64(5)).integers(-8, 9, (B, C) + tuple(size)).astype(np.float32)
    got, ref = _resize_bwd(dy, shape, size, nchw), _torch_resize_bwd(dy, shape, size)
    wrong = int((got != ref).sum())
    print(f"{shape}->{size} nchw={nchw}: {wrong} of {got.size} elements differ, max |dx| {np.abs(ref).max():.1f}")
    assert wrong == 0
    if tuple(size) == (h, w):
        assert np.array_equal(got, dy.transpose(0, 2, 3, 1))               # identity


@pytest.mark.parametrize("nchw", [True, False], ids=["dy_nchw", "dy_nhwc"])
@pytest.mark.parametrize("shape,size", R.RESIZE_GENERAL, ids=_ids)
def test_resize_bwd_general_ratio(shape, size, nchw):
    """|dx - torch| <= (n + 2) 2^-24 sum_i |w_i dy_i| per element; n and the sum from the index arithmetic in float64
    (tests/_seg_grad_ref.py: resize_bwd_bound)."""
    B, h, w, C = shape
    dy = np.random.Generator(np.random.PCG64(6)).standard_normal((B, C) + tuple(size)).astype(np.float32)
    got, ref = _resize_bwd(dy, shape, size, nchw), _torch_resize_bwd(dy, shape, size)
    bound = R.resize_bwd_bound(dy, h, w).transpose(0, 2, 3, 1)
    ratio = np.abs(got.astype(np.float64) - ref) / bound
    print(f"{shape}->{size} nchw={nchw}: worst error / bound = {ratio.max():.3f}, max abs error {np.abs(got - ref).max():.2e}")
    assert ratio.max() <= 1.0


@pytest.mark.parametrize("nchw", [True, False], ids=["y_nchw", "y_nhwc"])
@pytest.mark.parametrize("shape,size", R.RESIZE_EXACT[:2] + R.RESIZE_GENERAL, ids=_ids)
def test_resize_bwd_is_the_adjoint_of_the_forward_kernel(shape, size, nchw):
    """<y, dy> == <x, dx> with y from mv_resize_bilinear_nhwc_fwd and dx from the backward kernel, compared in float64.  Bound: the
    forward rounds each output at most 6 times relative to the sum of its taps' |x| (two differences, two products, two sums per
    axis pair), the backward as in the per-element bound, and either kernel's fp32 source coordinate (o + 1/2) in / out - 1/2 < in
    is off by at most 2^-22 in (quotient, product, difference), which moves each tap weight by as much."""
    B, h, w, C = shape
    H, W = size
    rng = np.random.Generator(np.random.PCG64(8))
    x = rng.standard_normal((B, h, w, C)).astype(np.float32)
    dy = rng.standard_normal((B, C, H, W)).astype(np.float32)
    xd = torch.from_numpy(x).cuda()
    y = torch.empty((B, C, H, W) if nchw else (B, H, W, C), dtype=torch.float32, device="cuda")
    _lib.call("mv_resize_bilinear_nhwc_fwd", _p(xd), _p(y), B, h, w, C, H, W, _lib.F32, _lib.F32, int(nchw), _stream())
    torch.cuda.synchronize()
    yh = y.cpu().numpy().astype(np.float64)
    yh = yh if nchw else yh.transpose(0, 3, 1, 2)
    dx = _resize_bwd(dy, shape, size, nchw).astype(np.float64)
    lhs, rhs = float((yh * dy).sum()), float((x * dx).sum())
    ax, ady = np.abs(x.astype(np.float64)).transpose(0, 3, 1, 2), np.abs(dy.astype(np.float64))
    Wy, Wx, Cy, Cx = R.tap_matrix(h, H), R.tap_matrix(w, W), R.tap_matrix(h, H, count=True), R.tap_matrix(w, W, count=True)
    fwd = lambda a, b, v: np.einsum("oi,bcij,pj->bcop", a, v, b)
    s_exact = float((ady * fwd(Wy, Wx, ax)).sum())
    s_taps = float((ady * fwd(Cy, Cx, ax)).sum())
    t = np.einsum("oi,bcop,pj->bcij", Wy, ady, Wx)
    n = np.einsum("oi,pj->ij", Cy, Cx)
    s_moved = float((ady * fwd(R.tap_matrix(h, H, extra=2.0 ** -22 * h), R.tap_matrix(w, W, extra=2.0 ** -22 * w), ax)).sum())
    bound = U * (6.0 * s_taps + float(((n + 2.0) * ax * t).sum())) + 2.0 * (s_moved - s_exact)
    print(f"{shape}->{size} nchw={nchw}: <y,dy> - <x,dx> = {lhs - rhs:.3e}, bound {bound:.3e}, |<y,dy>| {abs(lhs):.3e}")
    assert abs(lhs - rhs) <= bound


def test_resize_bwd_refuses_down_sampling(built_lib):
    d = torch.zeros(64, device="cuda")
    assert built_lib.mv_resize_bilinear_bwd_nhwc_f32(_p(d), _p(d), 1, 4, 4, 1, 2, 4, 0, None) == -1          # MV_E_INVALID
    assert b"down-sampling" in built_lib.mv_last_error()
    assert built_lib.mv_resize_bilinear_bwd_nhwc_f32(_p(d), _p(d), 1, 4, 4, 1, 4, 3, 1, None) == -1


# ------------------------------------------------------------------------------------------------ 2. per-pixel cross entropy
def _xent_map(logits, labels, where):
    """(loss [B,H,W], dlogits [B,C,H,W], sums [2]) from the kernel, run twice: bit-equal."""
    B, C, H, W = logits.shape
    ld = torch.from_numpy(logits).cuda()
    lab = torch.from_numpy(np.ascontiguousarray(labels.astype(np.int32))).cuda()
    md = None if where is None else torch.from_numpy(where.astype(np.uint8)).cuda()
    runs = []
    for _ in range(2):
        loss = torch.full((B * H * W + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
        dl = torch.full((B * C * H * W + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
        sums = torch.full((2 + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
        _lib.call("mv_softmax_xent_map_f32", _p(ld), _p(lab), _p(md), _p(loss), _p(dl), _p(sums), B, C, H * W, _stream())
        torch.cuda.synchronize()
        runs.append(torch.cat([loss, dl, sums]).cpu())
    assert torch.equal(runs[0].view(torch.int32), runs[1].view(torch.int32)), "two runs differ"
    loss, dl, sums = (t.cpu().numpy() for t in (loss, dl, sums))
    for buf, n in ((loss, B * H * W), (dl, B * C * H * W), (sums, 2)):
        assert (buf[n:] == SENTINEL).all(), "written past the end"
    return loss[:B * H * W].reshape(B, H, W), dl[:B * C * H * W].reshape(B, C, H, W), sums[:2]


def _xent_ref(logits, labels, where):
    t = torch.from_numpy(logits).double().requires_grad_(True)
    loss = R.pixel_losses(t, labels, where)
    loss.sum().backward()
    return loss.detach().numpy(), t.grad.numpy()


def _mask_case():
    rng = np.random.Generator(np.random.PCG64(2))
    where = np.zeros((2, 5, 7), bool)
    where[0] = rng.permutation(35).reshape(5, 7) >= 11              # 11 of 35 pixels of image 0 (30 %) are masked, image 1 entirely
    return where


XENT = {"2x21x5x7": ((2, 21, 5, 7), 3.0, None), "1x3x1x65_one_past_a_wave": ((1, 3, 1, 65), 3.0, None),
        "2x21x5x7_where": ((2, 21, 5, 7), 3.0, _mask_case()), "2x21x5x7_logits_pm80": ((2, 21, 5, 7), 80.0, None)}


@pytest.mark.parametrize("case", list(XENT))
def test_softmax_xent_map(case):
    """loss, dlogits and sums within the bound tests/_cases.py: xent_adam_case applies to mv_softmax_xent_f32 (|err| <= 1e-3
    max(1, max |ref|)) of float64 F.cross_entropy and its autograd; masked pixels exactly 0, the count exactly the mask's sum."""
    (B, C, H, W), scale, where = XENT[case]
    rng = np.random.Generator(np.random.PCG64(1))
    logits = (rng.uniform(-scale, scale, (B, C, H, W)) if scale > 10 else scale * rng.standard_normal((B, C, H, W))).astype(np.float32)
    labels = rng.integers(0, C, (B, H, W))
    if where is not None:
        labels = np.where(where, labels, 255)                         # out of range under the mask: not an error
    loss, dl, sums = _xent_map(logits, labels, where)
    _lib.check_device_status()
    rl, rd = _xent_ref(logits, labels, where)
    parts = [_cmp(loss, rl, TOL_F32), _cmp(dl, rd, TOL_F32), _cmp(sums[:1], np.asarray([rl.sum()]), TOL_F32)]
    print(case, [(p["err"], p.get("lim")) for p in parts], "sums", sums)
    assert all(p["ok"] for p in parts), parts
    assert np.isfinite(loss).all() and np.isfinite(dl).all()
    count = B * H * W if where is None else int(where.sum())
    assert sums[1] == count
    if where is not None:
        assert (loss[~where] == 0).all() and (dl.transpose(0, 2, 3, 1)[~where] == 0).all()
        assert not where[1].any() and where[0].sum() == 24
    # the public loss on the same operands, no tape: per-pixel values, mean over ALL pixels, sum
    pl = eqv.optim.softmax_cross_entropy_with_integer_labels(logits, labels, axis=1, where=where)
    assert np.array_equal(pl.losses.cpu().numpy(), loss)
    assert abs(pl.mean().item() - rl.mean()) <= TOL_F32 * max(1.0, abs(rl.mean()))
    assert abs(pl.sum().item() - rl.sum()) <= TOL_F32 * max(1.0, abs(rl.sum()))
    assert pl.counted == count


def test_softmax_xent_map_refuses_an_out_of_range_label_on_a_counted_pixel():
    rng = np.random.Generator(np.random.PCG64(3))
    logits = rng.standard_normal((2, 5, 3, 4)).astype(np.float32)
    labels = rng.integers(0, 5, (2, 3, 4))
    labels[1, 2, 1] = 5
    where = np.ones((2, 3, 4), bool)
    where[1, 2, 1] = False
    f = eqv.optim.softmax_cross_entropy_with_integer_labels
    _xent_map(logits, labels, where)                                    # under the mask: fine
    _lib.check_device_status()
    f(logits, torch.from_numpy(labels).cuda(), axis=1, where=where)
    _xent_map(logits, labels, None)                                     # counted: the status word says so, nothing was read out of bounds
    with pytest.raises(_lib.MVError, match="label outside"):
        _lib.check_device_status()
    _lib.check_device_status()                                          # cleared
    with pytest.raises(_lib.MVError, match="label outside"):
        f(logits, torch.from_numpy(labels).cuda(), axis=1)              # device labels: refused after the launch
    with pytest.raises(ValueError, match="label outside"):
        f(logits, labels, axis=1)                                       # host labels: refused before it
    labels[0, 0, 0] = -1
    with pytest.raises(ValueError, match="label outside"):
        f(logits, labels, axis=1, where=where)


# ------------------------------------------------------------------------------------------------ 3. models
def _build(name, sd=None, **kw):
    """The model of a case: loaded from the synthetic state in inference mode, or (sd None) fresh from its factory."""
    from eqxvision_amd.models.classification import resnet as RN
    model, aux, _ = R.CASES[name]
    if model == "lraspp":
        fac = lambda torch_weights=None, **k: eqv.models.lraspp_mobilenet_v3_large(torch_weights=torch_weights, num_classes=R.CLASSES, **k)
    else:
        bb = lambda: RN._resnet(RN._ResNetBottleneck, list(R.LAYERS), None, replace_stride_with_dilation=[False, True, True])
        make = eqv.models.fcn if model == "fcn" else eqv.models.deeplabv3
        tap = (lambda m: [m.layer3, m.layer4]) if aux else (lambda m: [m.layer4])
        fac = lambda torch_weights=None, **k: make(num_classes=R.CLASSES, backbone=bb(), intermediate_layers=tap,
                                                   aux_in_channels=1024 if aux else None, torch_weights=torch_weights, **k)
    return _load(fac, sd) if sd is not None else fac(**kw)


def _loss_fn(keys, where):
    xent = eqv.optim.softmax_cross_entropy_with_integer_labels

    @eqv.filter_value_and_grad
    def compute_loss(model, x, y):
        aux, out = eqv.vmap(model, axis_name="batch")(x, key=keys)
        loss = xent(out, y, axis=1, where=where).mean()
        if aux is not None:
            loss = loss + R.AUX_WEIGHT * xent(aux, y, axis=1, where=where).mean()
        return loss
    return compute_loss


@pytest.mark.parametrize("name", list(R.CASES))
def test_gradient_parity_with_autograd(name):
    """Inference mode (BatchNorm on stored statistics, Dropout off), B = 2, 64 x 64, 5 classes, fp32: grad_parity_case's criterion."""
    sd = R.case_state(name)
    x, labels, where = R.case_inputs(name)
    ref_loss, ref = R.reference(name)
    net = _build(name, sd)
    loss, grads = _loss_fn(_keys(R.B), where)(net, x, labels)
    got = eqv.utils.state_dict(grads)
    got_l = [(k, v) for k, v in got.items() if "running" not in k and np.asarray(v).dtype.kind == "f"]
    info = R.compare(got_l, [k for k in sd if k in ref], ref, loss, ref_loss)
    print(name, {k: info[k] for k in info if k != "over_lim"})
    if info.get("over_lim"):
        print(f"{name}: ReLU-flip allowance used for {info['over_lim']}")
    assert info["ok"], info


def test_unused_result_contributes_no_gradient():
    """A loss on `out` alone: the auxiliary head gets zeros, the rest the gradients of that loss; nothing raises."""
    name = "fcn_aux"
    sd = R.case_state(name)
    x, labels, _ = R.case_inputs(name)
    net = _build(name, sd)
    xent = eqv.optim.softmax_cross_entropy_with_integer_labels

    @eqv.filter_value_and_grad
    def only_out(model, xx, yy):
        _, out = eqv.vmap(model, axis_name="batch")(xx, key=_keys(R.B))
        return xent(out, yy, axis=1).sum() * (1.0 / labels.size)

    loss, grads = only_out(net, x, labels)
    got = eqv.utils.state_dict(grads)
    assert np.isfinite(loss)
    for k, v in got.items():
        if "running" in k or np.asarray(v).dtype.kind != "f":
            continue
        zero = not np.asarray(v).any()
        assert zero == k.startswith("aux_classifier."), k


@pytest.mark.parametrize("name", ["fcn_aux", "deeplabv3_aux", "lraspp"])
def test_two_adam_steps_in_training_mode(name):
    """The model straight from its factory (BatchNorm on batch statistics, Dropout live), two Adam steps in the shape of
    tests/_grad_cases.py: train_step_case: finite losses, every float leaf moves in the first step, the second loss differs."""
    net = _build(name, key=eqv.random.PRNGKey(0))
    x, labels, _ = R.case_inputs(name)
    opt = eqv.optim.adam(learning_rate=0.01)
    st = opt.init(eqv.filter(net, eqv.is_array))
    fn = _loss_fn(eqv.random.split(eqv.random.PRNGKey(1), R.B), None)
    floats = lambda m: [np.array(l, copy=True) for l in eqv.tree_leaves(m) if eqv.is_array(l) and l.dtype.kind == "f"]
    before, losses, stuck = floats(net), [], None
    for step in range(2):
        loss, grads = fn(net, x, labels)
        updates, st = opt.update(grads, st)
        net = eqv.apply_updates(net, updates)
        losses.append(loss)
        if step == 0:
            after = floats(net)
            stuck = [i for i, (a, b) in enumerate(zip(before, after)) if np.array_equal(a, b)]
    print(name, "losses", losses, "leaves", len(before), "not moved", stuck)
    assert all(np.isfinite(l) for l in losses)
    assert len(after) == len(before) and not stuck
    assert losses[1] != losses[0]
