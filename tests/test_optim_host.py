"""CPU side of the one-launch optimisers: the schedules against their closed forms, the host record plan, the refusals (chain,
adamw without params, a filter spec of another structure), and the proof that the bound test_optim_gpu.py applies passes an fp32
emulation of the kernels and sees each of its defects (tests/_optim_ref.py)."""
import functools
import math

import numpy as np
import pytest

import eqxvision_amd as eqv
from tests import _optim_ref as R

opt = eqv.optim


def test_constant_and_cosine_schedules():
    assert [opt.constant_schedule(0.3)(c) for c in (0, 1, 7)] == [0.3] * 3
    s = opt.cosine_decay_schedule(0.1, 10, alpha=0.2)
    for c in (0, 1, 5, 10, 11, 1000):
        want = 0.1 * (0.8 * 0.5 * (1 + math.cos(math.pi * min(c, 10) / 10)) + 0.2)
        assert s(c) == pytest.approx(want, rel=1e-15, abs=0)
        assert s(c) == pytest.approx(float(R.cosine64(c, 0.1, 10, 0.2)), rel=1e-15)
    assert s(0) == pytest.approx(0.1, rel=1e-15) and s(10) == pytest.approx(0.02, rel=1e-14) and s(25) == s(10)
    with pytest.raises(ValueError):
        opt.cosine_decay_schedule(0.1, 0)


def test_warmup_cosine_schedule():
    init, peak, warm, decay, end = 0.01, 0.5, 4, 20, 0.05
    s = opt.warmup_cosine_decay_schedule(init, peak, warm, decay, end)
    for c in (0, 1, warm - 1, warm, warm + 1, decay, decay + 7):
        if c < warm:
            want = init + (peak - init) * c / warm
        else:
            t = min(c - warm, decay - warm) / (decay - warm)
            want = end + (peak - end) * 0.5 * (1 + math.cos(math.pi * t))
        assert s(c) == pytest.approx(want, rel=1e-14), c
        assert s(c) == pytest.approx(float(R.warmup_cosine64(c, init, peak, warm, decay, end)), rel=1e-14)
    assert s(0) == init and s(warm) == pytest.approx(peak) and s(decay) == pytest.approx(end) and s(decay + 7) == s(decay)


def test_first_update_uses_schedule_of_zero():
    from eqxvision_amd import _optim
    s = opt.cosine_decay_schedule(1.0, 4)
    assert [_optim.rate(s, c) for c in range(3)] == [s(0), s(1), s(2)] and _optim.rate(s, 0) == 1.0
    assert _optim.rate(0.25, 17) == 0.25
    assert R.rates(3) == [float(R.cosine64(c, R.LR_INIT, R.LR_STEPS)) for c in (0, 1, 2)]


def test_record_plan():
    from eqxvision_amd import _optim
    sizes = [int(np.prod(s)) for s in R.SIZES]
    first, total = _optim.plan(sizes)
    blocks = [1, 1, 1, 1, 1, 1, 2, 3, 1] + [1] * 300 + [1]
    assert R.n_blocks() == blocks
    assert total == sum(blocks) == 6 + 2 + 3 + 1 + 300 + 1
    assert first == [sum(blocks[:i]) for i in range(len(blocks))]
    assert first[:10] == [0, 1, 2, 3, 4, 5, 6, 8, 11, 12]
    assert _optim.plan([4096 * 5 + 1]) == ([0], 6)
    with pytest.raises(ValueError):
        _optim.plan([4, 0])


def test_leaf_index_pairs_positions():
    from eqxvision_amd import _optim
    tree = {"a": np.zeros((2, 3), np.float32), "b": None, "c": 7, "d": [np.zeros(5, np.float32), np.arange(3)]}
    index, sizes = _optim.leaf_index(tree)
    assert index == [0, -1, -1, 1, -1] and sizes == [6, 5]
    assert len(eqv.tree_leaves(tree)) == 4 and len(eqv.tree_leaves(tree, none_is_leaf=True)) == 5


def test_chain_refusals():
    clip, sgd, adamw, adam = opt.clip_by_global_norm(1.0), opt.sgd(0.1), opt.adamw(0.1), opt.adam(0.1)
    for good in ((sgd,), (adamw,), (adam,), (clip, sgd), (clip, adamw), (clip, adam)):
        opt.chain(*good)
    for bad in ((), (clip,), (sgd, clip), (clip, clip, sgd), (sgd, adamw), (clip, sgd, adam), (clip, "sgd")):
        with pytest.raises(ValueError, match="clip_by_global_norm.*sgd.*adamw.*adam"):
            opt.chain(*bad)
    with pytest.raises(ValueError):
        opt.clip_by_global_norm(0.0)


def test_adamw_needs_params():
    o = opt.adamw(1e-3)
    assert o.wd == 1e-4 and (o.b1, o.b2, o.eps) == (0.9, 0.999, 1e-8)
    with pytest.raises(ValueError, match="params"):
        o.update({"w": None}, {"count": 0, "index": [-1], "mu": [], "nu": []})
    with pytest.raises(ValueError, match="params"):
        opt.chain(opt.clip_by_global_norm(1.0), o).update({"w": None}, {"count": 0, "index": [-1], "mu": [], "nu": []})


def test_spec_mismatch_is_a_value_error_before_the_device():
    net = eqv.models.resnet18(num_classes=3)
    other = eqv.tree_map(lambda _: False, eqv.models.resnet34(num_classes=3))
    called = []

    def loss(model, x):
        called.append(1)

    fn = functools.partial(eqv.filter_value_and_grad, arg=other)(loss)
    with pytest.raises(ValueError, match="spec does not match the model at .layer1"):
        fn(net, None)
    spec = eqv.tree_map(lambda _: False, net)
    spec = eqv.tree_at(lambda t: t.fc.weight, spec, replace="yes")
    with pytest.raises(ValueError, match="fc.weight"):
        eqv.filter_value_and_grad(loss, arg=spec)(net, None)
    assert not called


def test_filter_spec_built_as_in_the_tutorial():
    from eqxvision_amd.grad import _float_leaf, _frozen_ids
    net = eqv.models.resnet18(num_classes=3)
    spec = eqv.tree_map(lambda _: False, net)
    spec = eqv.tree_at(lambda t: (t.fc.weight, t.fc.bias), spec, replace=(True, True))
    assert spec.fc.weight is True and spec.fc.bias is True and spec.conv1.weight is False
    floats = [l for l in eqv.tree_leaves(net) if _float_leaf(l)]
    frozen = _frozen_ids(net, spec)
    assert len(frozen) == len(floats) - 2 and id(net.fc.weight) not in frozen and id(net.fc.bias) not in frozen
    by_module = eqv.tree_at(lambda t: t.fc, eqv.tree_map(lambda _: False, net), replace_fn=lambda fc: eqv.tree_map(lambda _: True, fc))
    assert _frozen_ids(net, by_module) == frozen
    assert _frozen_ids(net, True) == set() and len(_frozen_ids(net, False)) == len(floats)
    # the decorator forms
    assert callable(eqv.filter_value_and_grad(arg=spec)) and callable(functools.partial(eqv.filter_value_and_grad, arg=spec)(lambda m: 0))


@pytest.fixture(scope="module")
def data():
    return R.tensor_set()


@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("rule", list(R.RULES))
def test_bound_passes_the_emulation(data, rule, clip):
    params, grads = data
    mn = R.MAX_NORM if clip else None
    ref = R.reference(rule, params, grads, mn)
    ok, worst, failed = R.check_run(rule, clip, *R.emulate(rule, params, grads, mn), ref)
    print(f"{rule} clip={clip}: worst ratio {worst:.3f}")
    assert ok, failed


@pytest.mark.parametrize("defect,rule,clip", [("nesterov_ignored", "sgd_nesterov", False), ("wd_coupled", "adamw_wd05", False),
                                              ("count_minus_1", "adamw_wd0", False), ("clip_inverted", "sgd", True),
                                              ("clip_inverted", "adamw_wd05", True), ("schedule_at_count", "sgd_momentum", False),
                                              ("schedule_at_count", "adamw_wd0", False), ("tail_dropped", "sgd", False),
                                              ("tail_dropped", "adamw_wd05", True)])
def test_bound_sees_each_defect(data, defect, rule, clip):
    params, grads = data
    mn = R.MAX_NORM if clip else None
    ok, worst, failed = R.check_run(rule, clip, *R.emulate(rule, params, grads, mn, defect=defect), R.reference(rule, params, grads, mn))
    print(f"{defect} on {rule}: worst ratio {worst:.3g}")
    assert not ok and set(R.DEFECTS) >= {defect}


def test_every_defect_has_a_proof():
    import inspect
    src = inspect.getsource(test_bound_sees_each_defect)
    assert all(f'"{d}"' in src for d in R.DEFECTS)


def test_sqnorm_bound_and_its_defects(data):
    """The global norm: the emulation within ops_bound of float64 (n_ops = the longest chain of additions + 1), a dropped tail
    outside it; the factor is exactly 1 below max_norm and the inverted comparison shows."""
    from tests import _strict as ST
    _, grads = data
    g = grads[0]
    want, n = R.sqnorm64(g), R.n_sqnorm(sum(R.n_blocks()))
    assert n == 16 + 6 + 3 + 2 + 6 + 3 + 1
    s, f = R.emu_sqnorm(g, 1.0)
    assert ST.check_bound(np.array([s], np.float64), np.array([want]), want, None, "fp32", n_ops=n)["ok"]
    assert float(f) == pytest.approx(1.0 / math.sqrt(want), rel=1e-5)
    # the bound sees one tensor's tail going missing once that tail is not negligible
    big = [a.copy() for a in g]
    big[1][2] = 40.0
    s_bad, _ = R.emu_sqnorm(big, 1.0, defect="tail_dropped")
    w2 = R.sqnorm64(big)
    assert not ST.check_bound(np.array([s_bad], np.float64), np.array([w2]), w2, None, "fp32", n_ops=n)["ok"]
    assert ST.check_bound(np.array([R.emu_sqnorm(big, 1.0)[0]], np.float64), np.array([w2]), w2, None, "fp32", n_ops=n)["ok"]
    assert float(R.emu_sqnorm(g, 1000.0)[1]) == 1.0 and R.scale64(g, 1000.0) == 1.0
    assert float(R.emu_sqnorm(g, 1000.0, defect="clip_inverted")[1]) != 1.0
