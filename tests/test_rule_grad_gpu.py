"""`-m gpu`: every backward rule of eqxvision_amd/grad.py against float64 autograd, probe by probe (tests/_rule_grad.py; the
preconditions and the proofs that the instruments see defects are in tests/test_rule_grad_host.py).

test_exact: integer / dyadic operands; the forward value and every parameter gradient EQUAL the float64 twin.
test_bounded: Gaussian operands; forward value, loss and every parameter gradient satisfy
    max|got - g64| <= K max(E32, 2^-22 max|g64|),  K = 8,  E32 = max|float32 twin - float64 twin| per tensor.
test_adam_three_steps: adam(0.01) + apply_updates against torch.optim.Adam in float64 under the same bound, leaf by leaf and step
by step; `count` advances, non-float leaves stay.
The worst ratio err / (K max(E32, floor)) of each probe is printed (`pytest -s`); 1.0 is the limit.

Measured on an MI355X (worst ratio over the forward value, the loss and all gradient tensors; no probe needed K > 8):
    conv_plain 0.125, conv_variants 0.078, conv_bn_act_res 0.156, conv_act_res 0.142, conv_res_offtape 0.084, fanout 0.134,
    bn_train 0.374, bn_train#2 0.775, linear_family 0.132, vit_block 0.178, tokens_cls 0.067, tokens_noextra 0.052,
    pool_flatten 0.051, dropout_vec 0.106, dropout_map 0.103, dropout_rows 0.085, droppath_seq 0.054, droppath_map 0.161,
    droppath_local 0.089, se_sigmoid 0.088, se_hsig 0.207, se_silu 0.125, maxpool 0.116, stem 0.205, swin_noshift 0.137,
    swin_shift 0.157, patch_merge 0.100, concat_offtape 0.115, resize 0.051, loss_xent 0.097, loss_pixel 0.145,
    adam steps 1-3 0.110 / 0.210 / 0.312
(bn_train#2 is the second call of the same model; every exact probe: 0 elements differ.)
"""
import numpy as np
import pytest
import torch

import eqxvision_amd as eqv
from eqxvision_amd import _lib
from tests import _rule_grad as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    _lib.load()
    _lib.check_device_status()
    yield
    _lib.check_device_status()


@pytest.mark.parametrize("name", list(R.EXACT))
def test_exact(name):
    case = R.Case(name, "int")
    ref = R.run_twin(case)
    got = R.run_hip(case)
    bad = R.exact_mismatches(got, ref)
    total = sum(v.size + sum(g.size for g in gs) for v, _, gs in got)
    print(f"{name}: {bad} of {total} elements differ")
    assert bad == 0
    for (_, loss, _), (_, l64, _, _) in zip(got, ref):
        assert loss == l64


@pytest.mark.parametrize("name", R.BOUNDED)
def test_bounded(name):
    case = R.Case(name, "gauss")
    r64, r32 = R.run_twin(case), R.run_twin(case, torch.float32)
    got = R.run_hip(case)
    ratios = R.bounded_ratios(got, r64, r32)
    for call, r in enumerate(ratios):
        print(f"{name} call {call}: worst ratio {max(r):.3f} (forward {r[0]:.3f}, loss {r[1]:.3f}, gradients {[round(v, 3) for v in r[2:]]})")
    assert max(max(r) for r in ratios) <= 1.0, ratios


def test_adam_three_steps():
    case = R.Case("loss_xent", "gauss")
    ref64, ref32 = R.adam_reference(case), R.adam_reference(case, dtype=torch.float32)
    net = case.model
    other = [l for l in eqv.tree_leaves(net) if not (eqv.is_array(l) and l.dtype.kind == "f")]
    opt = eqv.optim.adam(0.01)
    st = opt.init(eqv.filter(net, eqv.is_array))
    assert st["count"] == 0

    @eqv.filter_value_and_grad
    def fn(model, xx):
        out = eqv.vmap(model, axis_name="batch")(xx, key=case.keys)
        return eqv.optim.softmax_cross_entropy(out, eqv.optim.one_hot(case.labels, 5)).mean()

    for step in range(3):
        _, grads = fn(net, case.xs[0])
        updates, st = opt.update(grads, st)
        net = eqv.apply_updates(net, updates)
        assert st["count"] == step + 1
        leaves = [np.asarray(l, np.float64) for l in R.float_leaves(net)]
        assert len(leaves) == len(ref64[step])
        ratios = [R.ratio(a, b, c) for a, b, c in zip(leaves, ref64[step], ref32[step])]
        print(f"adam step {step + 1}: ratios {[round(v, 3) for v in ratios]}")
        assert max(ratios) <= 1.0, ratios
        now = [l for l in eqv.tree_leaves(net) if not (eqv.is_array(l) and l.dtype.kind == "f")]
        assert len(now) == len(other) and all(a is b or a == b for a, b in zip(now, other))
