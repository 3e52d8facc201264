"""`-m gpu`: the one-launch optimisers (csrc/optim.hip) against float64 torch.optim, leaf by leaf and step by step, under the
per-element bound of tests/_optim_ref.py (n_ops counted from the kernel source; its derivation and the proof that the bound sees
the defects are in _optim_ref.py / test_optim_host.py); the global norm's reproducibility; apply_updates and adam(schedule) bit for
bit against the per-leaf path; and the pruned backward pass of a frozen backbone.

The tensor set (R.SIZES): 1, 3, 4, 5 (the n % 4 tail), 4095 / 4096 / 4097 (the chunk boundary), 8193 (three blocks), a [7, 3, 3, 3]
leaf, 300 tensors of one element (the record search) and one tensor handed over as a view 4 bytes into its allocation (the
element-by-element path).
"""
import functools

import numpy as np
import pytest
import torch

import eqxvision_amd as eqv
from eqxvision_amd import _lib, _optim
from eqxvision_amd._module import DevArray
from tests import _optim_ref as R
from tests import _strict as ST

pytestmark = pytest.mark.gpu
opt = eqv.optim


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    _lib.load()
    _lib.check_device_status()
    yield
    _lib.check_device_status()


@pytest.fixture(scope="module")
def data():
    return R.tensor_set()


def _dev(arrays):
    """The set as a list tree of device leaves; tensor R.UNALIGNED is a view one float into its allocation."""
    out = []
    for i, a in enumerate(arrays):
        t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
        if i == R.UNALIGNED:
            base = torch.empty(t.numel() + 1, dtype=torch.float32, device="cuda")
            base[1:].copy_(t.reshape(-1))
            t = base[1:].reshape(t.shape)
            assert t.data_ptr() % 16 == 4 and t.is_contiguous()
        out.append(DevArray(t))
    return out


def _host(tree):
    return [np.asarray(l) for l in tree]


def _make(rule, clip):
    kind, hp = R.RULES[rule]
    lr = opt.cosine_decay_schedule(R.LR_INIT, R.LR_STEPS)
    o = opt.sgd(lr, **hp) if kind == "sgd" else opt.adamw(lr, b1=R.B1, b2=R.B2, eps=R.EPS, **hp)
    return opt.chain(opt.clip_by_global_norm(R.MAX_NORM), o) if clip else o


# n_ops per case (R.n_update / R.n_param at step 3; no clip -> with clip, n_g = 0 -> 27):
#   sgd, sgd_momentum, sgd_nesterov   update 14 -> 41, parameter 18 -> 45
#   adamw_wd0, adamw_wd05             update 31 -> 85, parameter 35 -> 89
@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("rule", list(R.RULES))
def test_three_steps_against_float64(data, rule, clip):
    params, grads = data
    assert R.n_grad(True, 313) == 27 and R.n_update("sgd", 3, 0) == 14 and R.n_update("adamw", 3, 0) == 31
    assert R.n_update("sgd", 3, 27) == 41 and R.n_update("adamw", 3, 27) == 85 and R.n_param("adamw", 3, 27) == 89
    ref = R.reference(rule, params, grads, R.MAX_NORM if clip else None)
    o = _make(rule, clip)
    net = _dev(params)
    st = o.init(net)
    ups, pars = [], []
    for s, g in enumerate(grads):
        updates, st = o.update(_dev(g), st, net)
        net = eqv.apply_updates(net, updates)
        assert st["count"] == s + 1
        ups.append(_host(updates))
        pars.append(_host(net))
    ok, worst, failed = R.check_run(rule, clip, ups, pars, ref)
    print(f"{rule} clip={clip}: worst ratio {worst:.3f}")
    assert ok, failed


def _sqnorm(g, max_norm):
    rows = [(t.dev.data_ptr(), 0, 0, 0, t.dev.data_ptr(), t.dev.numel()) for t in g]
    out = _optim.sqnorm({}, rows, max_norm)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("max_norm,clipped", [(1.0, True), (1000.0, False)])
def test_global_norm(data, max_norm, clipped):
    """Same bits twice; the sum within ops_bound of float64 with n_ops = the longest chain of additions + 1 = 37 (16 per lane, 6 + 3
    in the workgroup, 2 + 6 + 3 in the second launch over 313 partial sums); the factor is exactly 1 below max_norm."""
    g = _dev(data[1][0])
    a, b = _sqnorm(g, max_norm), _sqnorm(g, max_norm)
    assert a.tobytes() == b.tobytes()
    want, n = R.sqnorm64(data[1][0]), R.n_sqnorm(sum(R.n_blocks()))
    assert n == 37
    info = ST.check_bound(np.array([a[0]], np.float64), np.array([want]), want, None, "fp32", n_ops=n)
    print(f"sum {a[0]!r} vs {want!r}: ratio {info['worst']:.3f}; factor {a[1]!r}")
    assert info["ok"], info
    if clipped:
        f = R.scale64(data[1][0], max_norm)
        finfo = ST.check_bound(np.array([a[1]], np.float64), np.array([f]), f, None, "fp32", n_ops=R.n_grad(True, 313) - 1)
        assert finfo["ok"], finfo
    else:
        assert a[1] == np.float32(1.0)


def test_apply_updates_equals_the_per_leaf_add(data):
    params, grads = data
    net, ups = _dev(params), _dev(grads[0])
    ups[3], ups[7] = None, None
    calls = []
    orig = _lib.call
    _lib.call = lambda name, *a: (calls.append(name), orig(name, *a))[1]
    try:
        new = eqv.apply_updates(net, ups)
    finally:
        _lib.call = orig
    assert calls == ["mv_optim_step_f32"]
    assert new[3] is net[3] and new[7] is net[7]
    for i, (p, u, y) in enumerate(zip(net, ups, new)):
        if u is None:
            continue
        ref = torch.empty(p.dev.numel(), dtype=torch.float32, device="cuda")
        pa, ua = p.dev.clone(), u.dev.clone()                             # the reference entry gets aligned copies of the view
        _lib.call("mv_add_fwd", pa.data_ptr(), ua.data_ptr(), ref.data_ptr(), p.dev.numel(), _lib.ACT_NONE, _lib.F32,
                  torch.cuda.current_stream().cuda_stream)
        assert y is not p and y.shape == p.shape
        assert torch.equal(ref, y.dev.reshape(-1)), i
    # a host leaf of another float width keeps its dtype and the host sum
    mixed = eqv.apply_updates([np.ones(3, np.float64), net[1]], [np.full(3, 0.5, np.float32), ups[1]])
    assert mixed[0].dtype == np.float64 and np.array_equal(mixed[0], np.full(3, 1.5)) and torch.equal(mixed[1].dev, new[1].dev)


def test_adam_with_a_schedule_equals_adam_at_the_scheduled_rates(data):
    params, grads = data
    sched = opt.cosine_decay_schedule(0.02, 4)
    a = opt.adam(sched)
    sa = a.init(_dev(params))
    sb = opt.adam(0.5).init(_dev(params))
    for s, g in enumerate(grads):
        g = _dev(g)
        g[5] = None                                                       # a frozen leaf: skipped by both
        ua, sa = a.update(g, sa)
        ub, sb = opt.adam(sched(s)).update(g, sb)
        assert sa["count"] == sb["count"] == s + 1 and ua[5] is None and ub[5] is None
        for i, (x, y) in enumerate(zip(ua, ub)):
            if x is not None:
                assert torch.equal(x.dev, y.dev), (s, i)
    assert float(sa["mu"][5].abs().max()) == 0.0
    # the clip in front of adam: the gradients times the factor, then adam as it is alone
    ch = opt.chain(opt.clip_by_global_norm(R.MAX_NORM), opt.adam(0.01))
    g = _dev(grads[0])
    uc, _ = ch.update(g, ch.init(_dev(params)))
    f = np.float32(_sqnorm(g, R.MAX_NORM)[1])
    scaled = [DevArray(torch.from_numpy(np.asarray(t) * f).cuda()) for t in g]
    ud, _ = opt.adam(0.01).update(scaled, opt.adam(0.01).init(_dev(params)))
    assert all(torch.equal(x.dev, y.dev) for x, y in zip(uc, ud))


def test_frozen_backbone():
    """resnet18(num_classes=3), B = 2, 32 x 32, inference-mode BatchNorm, spec True on fc only: fc's gradients have the bits of the
    unfiltered call, every other gradient is None, the backward pass launches no convolution or BatchNorm gradient, and two steps of
    adam(cosine_decay_schedule) move fc and leave every backbone leaf the object it was."""
    from oracle import state as S
    from tests._model_cases import _load
    net = _load(eqv.models.resnet18, S.resnet_state(1, "basic", (2, 2, 2, 2), num_classes=3), num_classes=3)
    x, y = S.synthetic_images(2, 32, seed=3), np.asarray([1, 2])
    keys = eqv.random.split(eqv.random.PRNGKey(0), 2)

    def loss(model, xx, yy):
        out = eqv.vmap(model, axis_name="batch")(xx, key=keys)
        return opt.softmax_cross_entropy(out, opt.one_hot(yy, 3)).mean()

    spec = eqv.tree_at(lambda t: (t.fc.weight, t.fc.bias), eqv.tree_map(lambda _: False, net), replace=(True, True))
    full = eqv.filter_value_and_grad(loss)
    part = functools.partial(eqv.filter_value_and_grad, arg=spec)(loss)
    l0, g0 = full(net, x, y)
    calls = []
    orig = _lib.call
    _lib.call = lambda name, *a: (calls.append(name), orig(name, *a))[1]
    try:
        l1, g1 = part(net, x, y)
    finally:
        _lib.call = orig
    assert l1 == l0
    assert np.array_equal(np.asarray(g1.fc.weight), np.asarray(g0.fc.weight)) and np.array_equal(np.asarray(g1.fc.bias), np.asarray(g0.fc.bias))
    assert float(np.abs(np.asarray(g1.fc.weight)).max()) > 0
    rest = [l for l in eqv.tree_leaves(g1, none_is_leaf=True) if isinstance(l, DevArray)]
    assert len(rest) == 2
    for m, g in zip(eqv.tree_leaves(net, none_is_leaf=True), eqv.tree_leaves(g1, none_is_leaf=True)):
        if isinstance(m, np.ndarray) and m.dtype.kind == "f" and m is not net.fc.weight and m is not net.fc.bias:
            assert g is None
    banned = {"mv_conv2d_wgrad_nhwc_f32", "mv_conv2d_dgrad_nhwc_f32", "mv_bn_dgamma_f32", "mv_bn_train_dz_coef_f32"}
    assert "mv_conv2d_nhwc_fwd" in calls and not banned & set(calls), sorted(banned & set(calls))

    o = opt.adam(opt.cosine_decay_schedule(1e-2, 10))
    st = o.init(eqv.filter(net, eqv.is_array))
    cur = net
    for _ in range(2):
        _, g = part(cur, x, y)
        updates, st = o.update(g, st)
        cur = eqv.apply_updates(cur, updates)
    before, after = eqv.tree_leaves(net, none_is_leaf=True), eqv.tree_leaves(cur, none_is_leaf=True)
    assert len(before) == len(after)
    moved = 0
    for a, b in zip(before, after):
        if a is net.fc.weight or a is net.fc.bias:
            assert b is not a and not np.array_equal(np.asarray(a), np.asarray(b))
            moved += 1
        else:
            assert b is a
    assert moved == 2 and st["count"] == 2
