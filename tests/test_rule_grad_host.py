"""CPU half of the rule-level gradient tests (tests/_rule_grad.py; the device half is tests/test_rule_grad_gpu.py).

grad.py cannot run without a device, so everything here is shown on the torch twin:
  * the rule -> probe table names every entry of grad.HOOKED, and every probe it names exists;
  * instrument 1's preconditions: every intermediate, gradient and absolute-value counterpart of the integer probes is a multiple
    of the stated dyadic unit below 2^24, fewer than 90 % of any gradient tensor is zero, no max-pool window holds a tie;
  * instrument 2's preconditions: no ReLU-family pre-activation and no max-pool window of the float64 reference is closer to a
    branch point than 2^-10 max|.|, no reference gradient tensor is identically zero, the float32 yardstick is finite;
  * the twin's entries equal oracle/np_ops.py where the oracle has the op;
  * every defect switch of the twin is rejected: by inequality on the exact probes, by the bound (with the true E32) on the others."""
import re

import numpy as np
import pytest
import torch

from oracle import np_ops as O
from tests import _rule_grad as R

RESTATEMENT_TOL = 3e-7          # numpy == torch restatement, relative to max |.| (tests/test_seg_grad_host.py, tests/test_oracle.py)


@pytest.fixture(scope="module")
def refs():
    """(probe, kind) -> (case, float64 runs, float32 runs), computed once and left unchanged."""
    cache = {}

    def get(name, kind):
        if (name, kind) not in cache:
            case = R.Case(name, kind)
            cache[name, kind] = (case, R.run_twin(case), R.run_twin(case, torch.float32) if kind == "gauss" else None)
        return cache[name, kind]
    return get


def test_rule_table_names_every_hooked_entry():
    from eqxvision_amd import grad
    rows = dict(re.findall(r"^    (\w+) +([\w, ]+)$", R.__doc__, re.M))
    assert set(rows) == set(grad.HOOKED), (set(grad.HOOKED) - set(rows), set(rows) - set(grad.HOOKED))
    for rule, probes in rows.items():
        names = [p.strip() for p in probes.split(",")]
        assert names and all(p in R.PROBES for p in names), (rule, names)
    assert set(R.EXACT) | set(R.BOUNDED) == set(R.PROBES) and set(R.BODY) == set(R.PROBES)
    assert set(R.DEFECT_PROBES) | {"adam_count_minus_1"} == set(R.DEFECTS)


@pytest.mark.parametrize("name", list(R.EXACT))
def test_exact_preconditions(name):
    case = R.Case(name, "int")
    ref = R.prove_probe_exact(case)
    for _, _, _, tw in ref:
        assert all(act == "relu" for act, _ in tw.branches)
        if tw.pools:                                    # no window holds a tie: the tie rule belongs to the kernel tests
            gaps = R.Twin(case.model)
            gaps.pools = tw.pools
            assert R.margins(gaps) > 0


@pytest.mark.parametrize("name", R.BOUNDED)
def test_bounded_preconditions(name, refs):
    case, r64, r32 = refs(name, "gauss")
    for (v, l, grads, tw), (v32, l32, g32, _) in zip(r64, r32):
        m = R.margins(tw)
        print(f"{name}: margin {m:.2e} (required {R.MARGIN:.2e})")
        assert m >= R.MARGIN
        assert np.isfinite(v32).all() and all(np.isfinite(g).all() for g in g32)
        for i, g in enumerate(grads):
            assert g.any(), f"{name}: reference gradient {i} is identically zero"
            assert R.ratio(g32[i], g, g32[i], k=1) <= 1.0        # the yardstick passes its own criterion


def test_drop_path_keys_keep_and_drop():
    for name in ("droppath_seq", "droppath_map", "droppath_local"):
        case = R.Case(name, "gauss")
        kept = [bool(O.jax_bernoulli(k, np.float32(0.5))) for k in case.keys]
        assert any(kept) and not all(kept), (name, kept)
    local = np.stack([O.jax_bernoulli(k, np.float32(0.5), (8,)) for k in R.Case("droppath_local", "gauss").keys])
    assert all(r.any() and not r.all() for r in local)              # every sample keeps some channels and drops some


# ------------------------------------------------------------------------------------------------ twin == numpy oracle
def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.abs(a - b).max() / max(1e-30, np.abs(b).max()))


def _twin(model):
    return R.Twin(model)


def test_twin_entries_equal_the_numpy_oracle():
    rng = np.random.Generator(np.random.PCG64(3))
    from eqxvision_amd import nn
    x = rng.standard_normal((2, 4, 6, 5)).astype(np.float32)
    keys = R.jr.split(R.jr.PRNGKey(5), 2)
    errs = {}
    conv = nn.Conv2d(4, 6, 3, stride=(2, 1), padding=1, dilation=(1, 2), groups=2)
    lin = nn.Linear(5, 7)
    ln = nn.LayerNorm(5)
    bn = R._bn_inf(4, rng)
    bnt = nn.BatchNorm(4, "batch")
    L = {"conv": conv, "lin": lin, "ln": ln, "bn": bn, "bnt": bnt}
    R._fill(L, rng, "gauss")
    tw = _twin(R.Probe(L, None))
    a = tw.as_map(tw.input(x))
    errs["conv2d"] = _rel(tw.conv2d(a, conv).t.detach(), O.vmap(lambda s: O.conv2d(s, conv.weight, conv.bias, conv.stride, conv.padding, conv.dilation, 2))(x))
    errs["bn_inference"] = _rel(tw.batchnorm(a, bn).t.detach(), O.vmap(lambda s: O.batchnorm_inference(s, bn.weight, bn.bias, *bn.state_index.value))(x))
    y1, run = O.batchnorm_train(x, bnt.weight, bnt.bias, None, True)
    errs["bn_train_first"] = _rel(tw.batchnorm(a, bnt).t.detach(), y1)
    y2, _ = O.batchnorm_train(x[::-1], bnt.weight, bnt.bias, run, False)
    errs["bn_train_second"] = _rel(tw.batchnorm(tw.input(x[::-1].copy()), bnt).t.detach(), y2)
    rows = tw.input(x)
    rows = R.TA(rows.t.reshape(2, 24, 5), "seq")
    errs["linear"] = _rel(tw.linear(rows, lin).t.detach(), x.reshape(2, 24, 5) @ lin.weight.T + lin.bias)
    errs["layernorm"] = _rel(tw.layernorm(rows, ln).t.detach(), O.vmap(lambda s: O.layernorm_rows(s, ln.weight, ln.bias))(x.reshape(2, 24, 5)))
    errs["maxpool2d"] = _rel(tw.maxpool2d(a, 3, 2, 1).t, O.vmap(lambda s: O.maxpool2d(s, 3, 2, 1))(x))
    errs["avgpool"] = _rel(tw.adaptive_avgpool2d(a, (1, 1)).t, O.vmap(lambda s: O.adaptive_avgpool2d(s, 1))(x))
    errs["resize"] = _rel(tw.resize_bilinear(a, (12, 10)).t, O.vmap(lambda s: O.resize_bilinear(s, (12, 10)))(x))
    for act, fn in (("relu", O.relu), ("gelu", O.gelu_tanh), ("silu", O.silu), ("sigmoid", O.sigmoid), ("hard_sigmoid", O.hard_sigmoid),
                    ("hard_swish", O.hard_swish)):
        errs[act] = _rel(tw.eltwise(a, act).t, fn(x))
    errs["dropout_map"] = _rel(tw.dropout(a, 0.5, keys).t, np.stack([O.dropout(s, 0.5, k) for s, k in zip(x, keys)]))
    for mode in ("global", "local"):
        errs["drop_path_" + mode] = _rel(tw.drop_path(a, 0.5, mode, keys).t, np.stack([O.drop_path(s, 0.5, mode, k) for s, k in zip(x, keys)]))
    tok_rows = x.reshape(2, 24, 5)
    per_row = np.stack([np.stack([O.dropout(r, 0.5, k) for r, k in zip(s, O.jax_split(key, 24))]) for s, key in zip(tok_rows, keys)])
    errs["dropout_rows"] = _rel(tw.dropout(rows, 0.5, keys, per_row=True).t, per_row)
    merged = tw.patch_merge_gather(tw.input(x[:, :, :, :4].copy())).t.numpy()
    s = x[0, :, :, :4]
    errs["patch_merge"] = _rel(merged[0], np.concatenate([s[:, 0::2, 0::2], s[:, 1::2, 0::2], s[:, 0::2, 1::2], s[:, 1::2, 1::2]], 0))
    # attention: the oracle's functions include the projections
    D, heads = 8, 2
    t = rng.standard_normal((2, 7, D)).astype(np.float32)
    qkv, proj = nn.Linear(D, 3 * D), nn.Linear(D, D)
    rel = R.RelBias((2, 3), heads)
    LA = {"qkv": qkv, "proj": proj, "rel": rel}
    R._fill(LA, rng, "gauss")
    twa = _twin(R.Probe(LA, None))
    got = twa.linear(twa.qkv_attention(R.TA(torch.from_numpy(t).double(), "seq"), qkv, heads, 0.5), proj).t.detach()
    errs["vit_attention"] = _rel(got, O.vmap(lambda s: O.vit_attention(s, qkv.weight, qkv.bias, proj.weight, proj.bias, heads)[0])(t))
    m = rng.standard_normal((2, D, 4, 6)).astype(np.float32)
    bias = O.relative_position_bias(rel.relative_position_bias_table, rel.relative_position_index, (2, 3))
    assert np.asarray(rel.relative_position_index).min() < 0
    for shift in ((0, 0), (1, 1)):
        mm = R.TA(torch.from_numpy(m).double(), "map")
        got = twa.linear(twa.swin_attention(twa.linear(mm, qkv), rel, heads, (2, 3), shift), proj).t.detach()
        ref = O.vmap(lambda s: O.shifted_window_attention(s, qkv.weight, proj.weight, bias, (2, 3), heads, shift, qkv.bias, proj.bias))(m)
        errs[f"swin_attention_shift{shift[0]}"] = _rel(got, ref)
    print({k: f"{v:.1e}" for k, v in errs.items()})
    bad = {k: v for k, v in errs.items() if v > RESTATEMENT_TOL}
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ the instruments see defects
def _rejected(name, kind, defect, refs):
    case, r64, r32 = refs(name, kind)
    bad = R.run_twin(case, defect=defect)
    got = [(v, l, g) for v, l, g, _ in bad]
    if kind == "int":
        n = R.exact_mismatches(got, r64)
        return n > 0, f"{n} elements differ"
    worst = max(max(r) for r in R.bounded_ratios(got, r64, r32))
    return worst > 1.0, f"worst ratio {worst:.3g}"


@pytest.mark.parametrize("defect,name", [(d, p) for d, ps in R.DEFECT_PROBES.items() for p in ps])
def test_defect_is_rejected(defect, name, refs):
    for kind in (["int"] if name in R.EXACT else []) + (["gauss"] if name in R.BOUNDED else []):
        ok, what = _rejected(name, kind, defect, refs)
        print(f"{defect} on {name}/{kind}: {what}")
        assert ok, f"{defect} on {name}/{kind} passes the instrument ({what})"
    # and the forward value is untouched: the defect lives in the backward pass alone
    case, r64, _ = refs(name, "gauss" if name in R.BOUNDED else "int")
    for (v, *_), (vd, *_) in zip(r64, R.run_twin(case, defect=defect)):
        assert np.allclose(v, vd, rtol=1e-12, atol=1e-12)


def test_adam_reference_and_its_defect():
    case = R.Case("loss_xent", "gauss")
    ref64, ref32 = R.adam_reference(case), R.adam_reference(case, dtype=torch.float32)
    start = [np.asarray(l, np.float64) for l in R.float_leaves(case.model)]
    for step, leaves in enumerate(ref64):
        assert all(np.isfinite(a).all() for a in leaves)
        moved = [float(np.abs(a - b).max()) for a, b in zip(leaves, start)]
        assert all(m > 0 for m in moved), moved
    for sa, sb in zip(ref64, R.adam_reference(case, written_out=True)):        # the written-out update the defect is a switch of
        assert all(np.allclose(a, b, rtol=1e-12, atol=1e-14) for a, b in zip(sa, sb))
    bad = R.adam_reference(case, defect="adam_count_minus_1")
    worst = max(R.ratio(b, a, c) for sb, sa, sc in zip(bad, ref64, ref32) for b, a, c in zip(sb, sa, sc))
    print(f"adam_count_minus_1: worst ratio {worst:.3g}")
    assert worst > 1.0
