"""`-m gpu`: the mixed-precision Linear kernels (csrc/linear_mp.hip: mv_linear_mp_fwd / _dgrad / _wgrad) and the rule that uses them
(filter_value_and_grad(..., matmul_dtype="bf16")).  References, roundings and case generators: tests/_linear_mp_ref.py; the CPU proof
that the cases see a wrong rounding, fp32 products and a rounded bias: tests/test_linear_mp_host.py.

Every destination is sentinel-filled with a guard behind it, the serving kernel is asserted (`_lib.last_kernel()`), references are
float64 on the bf16-rounded operands.

1. exact, integers in [-2, 2], the seven shapes of R.SHAPES (odd K / N: the 4-byte load path; (1, 1, 1): a tile that is all edge).
2. exact with the rounding visible: operands k 2^-10 with every tie, reduction 16, a bias that is no bf16 value.
3. wgrad under every scratch regime: bit-equal, bytes [0, 4096) of the offer left zero; an offer it does not take stays on offer.
4. Gaussian operands within S.elem_bound(ref, mag, kred, "fp32"), kred = the reduction length: holds for any summation order (a tree over
   n terms is at most n - 1 deep, so the split adds no term).
5. the rule: g_linear under "bf16" (y, dx, dW, db; a frozen weight launches no wgrad; the head stays on the fp32 kernel).
6. a model: vit (32 x 32, depth 2) against a float64 emulation that rounds x, w and the incoming gradient of every Linear but `fc`.

Measured on an MI355X, worst |got - ref| / bound per entry over the shapes of case 4 (every exact case was bit-equal, under every
scratch regime):
    fwd    0.033 (64 x 128 x 16)
    dgrad  0.005 (257 x 96 x 40, 256 x 128 x 64, 788 x 192 x 768)
    wgrad  0.010 (33 x 17 x 9); split in three parts at 788 x 192 x 768: below 0.001
    rule   y 0.014, dx 0.009, dW 0.004, db 0.006
    model  relative L2 of the device under "bf16" against (b) 1.267e-06; (b) against (a) 2.111e-03: ratio 0.0006 (allowed 0.25); the
           device's fp32 path against (a) 1.465e-07
"""
import contextlib
import types

import numpy as np
import pytest
import torch

from eqxvision_amd import _lib
from tests import _linear_mp_ref as R
from tests import _strict as S
from tests._cases import TOL_F32, _cmp
from tests._strict_gpu import _Flags, _need_gpu, _p, _stream  # noqa: F401  (_need_gpu: the module fixture)
from tests.test_strict_bwd_gpu import AMPLE, SYNC, _f, _Scratch
from tests.test_strict_mem_gpu import _judge, _run

pytestmark = pytest.mark.gpu
F64 = np.float64
KERNEL = {"fwd": "linear_mp_fwd_bf16", "dgrad": "linear_mp_dgrad_bf16", "wgrad": "linear_mp_wgrad_bf16"}
SPLIT = "linear_mp_wgrad_split_bf16"
IDS = [R.shape_id(s) for s in R.SHAPES]


def _launch(entry, M, N, K, x, w, g, bias=None, offer=None):
    """One launch on a sentinel-filled, guarded destination -> (values as float64, kernel name)."""
    xd, wd, gd = (None if a is None else _f(a) for a in (x, w, g))
    bd = None if bias is None else _f(bias)
    with _Scratch(offer):
        if entry == "fwd":
            return _run("mv_linear_mp_fwd", lambda y: (_p(xd), _p(wd), _p(bd), y, M, N, K, _stream()), (M, N), "fp32")
        if entry == "dgrad":
            return _run("mv_linear_mp_dgrad", lambda y: (_p(gd), _p(wd), y, M, N, K, _stream()), (M, K), "fp32")
        return _run("mv_linear_mp_wgrad", lambda y: (_p(gd), _p(xd), y, M, N, K, _stream()), (N, K), "fp32")


# ================================================================================================ 1. exact, integers
@pytest.mark.parametrize("entry", R.ENTRIES)
@pytest.mark.parametrize("shape", R.SHAPES, ids=IDS)
def test_exact_int(shape, entry):
    M, N, K = shape
    x, w, g, bias = R.int_case(M, N, K)
    for b in ((None, bias) if entry == "fwd" else (None,)):
        ref, mag = R.product_ref(entry, x, w, g, b)
        S.prove_exact(f"linear_mp/{entry}/{R.shape_id(shape)}", ref, mag, list(R._operands(entry, x, w, g)), out="fp32")
        got, kern = _launch(entry, M, N, K, x, w, g, b)
        _judge(f"linear_mp/{entry}/int/{R.shape_id(shape)}/{'bias' if b is not None else 'nobias'}", kern, KERNEL[entry], got, ref, "fp32")


# ================================================================================================ 2. exact, rounding visible
@pytest.mark.parametrize("entry", R.ENTRIES)
def test_exact_rounding(entry):
    M, N, K = R.round_shape(entry)
    x, w, g, bias = R.round_case(entry)
    ref, mag = R.product_ref(entry, x, w, g, bias)
    R.prove_round_case(entry, ref, mag, x, w, g, bias)
    got, kern = _launch(entry, M, N, K, x, w, g, bias if entry == "fwd" else None)
    _judge(f"linear_mp/{entry}/round/{M}x{N}x{K}", kern, KERNEL[entry], got, ref, "fp32")


# ================================================================================================ 3. wgrad, scratch regimes
WGRAD_N, WGRAD_K = 70, 40
WGRAD_M = [1030, 18145]               # 18145 = 63 parts of 288 rows + one row (R.wgrad_split; proved in test_linear_mp_host.py)


def _regimes(out_elems):
    return [("no_offer", None), ("ample", AMPLE), ("fit2", SYNC + int(2.5 * out_elems * 4)), ("fit1", SYNC + int(1.5 * out_elems * 4))]


@pytest.mark.parametrize("M", WGRAD_M)
def test_wgrad_scratch_regimes(M):
    N, K = WGRAD_N, WGRAD_K
    x, w, g, _ = R.int_case(M, N, K)
    ref, mag = R.product_ref("wgrad", x, w, g)
    S.prove_exact(f"linear_mp/wgrad/{M}", ref, mag, list(R._operands("wgrad", x, w, g)), out="fp32")
    results = []
    for name, offer in _regimes(N * K):
        parts = R.wgrad_split(M, N, K, offer)[1]
        got, kern = _launch("wgrad", M, N, K, x, w, g, offer=offer)          # (_Scratch asserts bytes [0, 4096) of the offer are zero)
        _judge(f"linear_mp/wgrad/M{M}/{name}/parts{parts}", kern, SPLIT if parts > 1 else KERNEL["wgrad"], got, ref, "fp32")
        results.append(got)
    for r in results[1:]:
        assert np.array_equal(r, results[0])


def test_wgrad_leaves_an_offer_it_does_not_take():
    """An offer with room for one part: mv_linear_mp_wgrad (1030 x 17 x 9 wants 4 parts) runs unsplit and only LOOKS at the offer, so the
    next launch on the stream, with no new mv_set_scratch, still finds it: mv_colsum_f32 on 515 x 2 (3 parts, 4096 + 24 bytes) splits."""
    M, N, K = 1030, 17, 9
    offer = SYNC + int(1.5 * N * K * 4)
    assert R.wgrad_split(M, N, K)[0] == 4 and R.wgrad_split(M, N, K, offer)[1] == 1
    assert SYNC + 24 <= offer < SYNC + 2 * N * K * 4 and S.colsum_split(515) == (3, 172)
    x, w, g, _ = R.int_case(M, N, K)
    ref, mag = R.product_ref("wgrad", x, w, g)
    S.prove_exact("linear_mp/wgrad/untaken", ref, mag, list(R._operands("wgrad", x, w, g)), out="fp32")
    a = S.int_tensor(S.rng_of(71), (515, 2), 2)
    xd, gd, ad = _f(x), _f(g), _f(a)
    with _Scratch(offer):
        got, kern = _run("mv_linear_mp_wgrad", lambda y: (_p(gd), _p(xd), y, M, N, K, _stream()), (N, K), "fp32")
        col, ckern = _run("mv_colsum_f32", lambda y: (_p(ad), None, y, 515, 2, _stream()), (2,), "fp32")
    _judge("linear_mp/wgrad/untaken_offer", kern, KERNEL["wgrad"], got, ref, "fp32")
    _judge("linear_mp/wgrad/untaken_offer/colsum_after", ckern, "colsum_split_f32", col, S.colsum_ref(a, None)[0], "fp32")


# ================================================================================================ 4. bounded, Gaussian
BOUND_IDS = [R.shape_id(s) for s in R.BOUND_SHAPES]


@pytest.mark.parametrize("entry", R.ENTRIES)
@pytest.mark.parametrize("shape", R.BOUND_SHAPES, ids=BOUND_IDS)
def test_bounded_gauss(shape, entry):
    M, N, K = shape
    x, w, g, bias = R.gauss_case(M, N, K)
    b = bias if entry == "fwd" else None
    ref, mag = R.product_ref(entry, x, w, g, b)
    bound = S.elem_bound(ref, mag, R.kred_of(entry, M, N, K), "fp32")
    offers = (None, AMPLE) if entry == "wgrad" else (None,)
    for offer in offers:
        parts = R.wgrad_split(M, N, K, offer)[1] if entry == "wgrad" else 1
        got, kern = _launch(entry, M, N, K, x, w, g, b, offer=offer)
        _judge(f"linear_mp/{entry}/gauss/{R.shape_id(shape)}/parts{parts}", kern, SPLIT if parts > 1 else KERNEL[entry], got, ref, "fp32",
               bound=bound)


# ================================================================================================ 5. the rule
@contextlib.contextmanager
def _calls():
    """The names of the C-ABI entries called inside the scope."""
    names, orig = [], _lib.call

    def call(name, *a):
        names.append(name)
        return orig(name, *a)
    _lib.call = call
    try:
        yield names
    finally:
        _lib.call = orig


def _leaf_act(leaf):
    """A parameter leaf as an activation on the tape: its gradient is the gradient that reaches the activation."""
    from eqxvision_amd import grad
    from eqxvision_amd._act import Act
    a = Act(grad._leaf_dev(leaf), "seq", True)

    def backward(g):
        grad._acc_param(leaf, g)
        return ()
    a.node = grad.Node([], backward)
    return a


def _rule(B, T, K, N, use_bias, extras, spec_freeze_weight=False, head=False, dtype="bf16"):
    """One nn.Linear on [B, T, K] rows (+ residual and gelu with `extras`) under matmul_dtype=`dtype`, the loss <y, G0>.
    Returns (operands, G0, y, grads as float64 arrays, the entries called)."""
    import eqxvision_amd as eqv
    from eqxvision_amd import nn, ops
    from tests._rule_grad import linear_loss
    rng = S.rng_of(31)
    lin = nn.Linear(K, N, use_bias=use_bias, key=eqv.random.PRNGKey(1))
    lin.weight = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    if use_bias:
        lin.bias = (0.1 * rng.standard_normal(N)).astype(np.float32)
    model = {"x0": rng.standard_normal((B, T, K)).astype(np.float32), "lin": lin}
    if extras:
        model["r0"] = rng.standard_normal((B, T, N)).astype(np.float32)
    G0 = rng.standard_normal((B, T, N)).astype(np.float32)
    seen = {}
    spec = None
    if spec_freeze_weight:
        spec = {k: True for k in model}
        spec["lin"] = eqv.tree_map(lambda l: l is not lin.weight, lin)

    @eqv.filter_value_and_grad(arg=spec, matmul_dtype=dtype)
    def fn(m):
        xa = _leaf_act(m["x0"])
        if head:
            y = ops.linear_head(xa, m["lin"])
        elif extras:
            y = ops.linear(xa, m["lin"], "gelu", _leaf_act(m["r0"]))
        else:
            y = ops.linear(xa, m["lin"])
        seen["y"] = y.t.detach().cpu().numpy().astype(F64)
        return linear_loss(types.SimpleNamespace(act=y), G0)

    with _calls() as names:
        _, grads = fn(model)
    g = {"x0": np.asarray(grads["x0"], F64), "w": None if grads["lin"].weight is None else np.asarray(grads["lin"].weight, F64)}
    if use_bias:
        g["b"] = np.asarray(grads["lin"].bias, F64)
    if extras:
        g["r0"] = np.asarray(grads["r0"], F64)
    return model, G0, seen["y"], g, names


def _within(tag, got, ref, bound):
    i = S.check_bound(got, ref, None, 0, "fp32", bound=bound)
    print(f"{tag}: worst |got-ref|/bound {i.get('worst', float('nan')):.3f} over {i.get('n')} elements, violations {i.get('nviol')}")
    assert i["ok"], (tag, i)


@pytest.mark.parametrize("use_bias,extras", [(True, False), (False, False), (True, True)], ids=["bias", "nobias", "bias_res_gelu"])
def test_rule(use_bias, extras):
    """B T = 3 x 67 rows of K = 40 to N = 72.  Without an activation the gradient the backward products round is G0 itself.  With the
    residual and gelu, g2 = G0 gelu'(z) is computed by mv_act_bwd_f32 from the DEVICE's z: g2 (it is the residual's gradient) is held
    to that kernel's own criterion (tests/test_strict_bwd_gpu.py: test_act_bwd), and dx, dW and db are referred to the device's g2, so
    that each product is held to the bound that follows from its own arithmetic."""
    B, T, K, N = 3, 67, 40, 72
    M = B * T
    model, G0, y, g, names = _rule(B, T, K, N, use_bias, extras)
    x, w = model["x0"].reshape(M, K), model["lin"].weight
    bias = model["lin"].bias if use_bias else None
    res = model["r0"].reshape(M, N) if extras else None
    r = R.rule_ref(x, w, bias, res, "gelu" if extras else None, G0.reshape(M, N))
    assert names.count("mv_linear_mp_fwd") == 1 and names.count("mv_linear_mp_wgrad") == 1 and names.count("mv_linear_mp_dgrad") == 1
    assert "mv_transpose2d_f32" not in names and "mv_linear_fwd" not in names
    assert names[names.index("mv_linear_mp_wgrad") - 1] == "mv_set_scratch"
    yref, zmag = r["y"]
    if extras:
        _, ybound = S.act_bound(r["z"], zmag, K, S.ACT_CODES["gelu_tanh"], "fp32")
    else:
        ybound = S.elem_bound(yref, zmag, K, "fp32")
    _within("rule/y", y.reshape(M, N), yref, ybound)
    g2 = G0.reshape(M, N).astype(np.float32)
    if extras:
        g2 = g["r0"].reshape(M, N).astype(np.float32)
        i = _cmp(g2.astype(F64), r["g2"], TOL_F32)
        print(f"rule/g2: max |got-ref| {i.get('err')} of {i.get('lim')} allowed")
        assert i["ok"], i
    dx, dxmag = R.product_ref("dgrad", w=w, g=g2)
    _within("rule/dx", g["x0"].reshape(M, K), dx, S.elem_bound(dx, dxmag, N, "fp32"))
    dw, dwmag = R.product_ref("wgrad", x=x, g=g2)
    _within("rule/dW", g["w"], dw, S.elem_bound(dw, dwmag, M, "fp32"))
    if use_bias:
        db, dbmag = g2.astype(F64).sum(0), np.abs(g2.astype(F64)).sum(0)
        _within("rule/db", g["b"], db, S.ops_bound(db, dbmag, S.colsum_n_ops(M, 1), "fp32"))


def test_rule_frozen_weight_launches_no_wgrad():
    model, G0, y, g, names = _rule(2, 33, 24, 40, True, False, spec_freeze_weight=True)
    assert "mv_linear_mp_wgrad" not in names and names.count("mv_linear_mp_dgrad") == 1 and names.count("mv_linear_mp_fwd") == 1
    assert g["w"] is None and np.abs(g["x0"]).max() > 0 and np.abs(g["b"]).max() > 0


def test_rule_head_stays_fp32():
    """g_linear_head under "bf16": the fp32 entries of the default path, launch for launch, and its values."""
    a = _rule(2, 33, 24, 5, True, False, head=True, dtype="bf16")
    b = _rule(2, 33, 24, 5, True, False, head=True, dtype="fp32")
    assert not any(n.startswith("mv_linear_mp") for n in a[4]) and a[4].count("mv_linear_fwd") == 3
    assert a[4] == b[4]
    assert np.array_equal(a[2], b[2]) and all(np.array_equal(a[3][k], b[3][k]) for k in a[3])


def test_default_is_fp32_path():
    """No keyword: the launches of the parent commit (two transposes and mv_linear_fwd for dW, mv_linear_fwd on the cached transpose for dx)."""
    names = _rule(2, 33, 24, 40, True, False, dtype="fp32")[4]
    assert not any(n.startswith("mv_linear_mp") for n in names)
    assert names.count("mv_linear_fwd") == 3 and names.count("mv_transpose2d_f32") == 3


# ================================================================================================ 6. a model
def _flat(sd_like, names):
    return np.concatenate([np.asarray(sd_like[n], F64).reshape(-1) for n in names])


def test_vit_model():
    """vit 32 x 32, patch 8, width 64, depth 2, 2 heads, 5 classes, B = 2 (the configuration of jit_train_loop_case).  (a) float64, (b) float64
    with every Linear but `fc` rounding x, w and the incoming gradient, (c) the device's fp32 path.  The device under "bf16" may differ from
    (b) only by fp32 summation order and the few values that this pushes across a bf16 rounding boundary: its relative L2 distance to
    (b) must be at most a quarter of the distance of (b) to (a), the effect of the rounding itself."""
    import eqxvision_amd as eqv
    from tests._model_cases import _keys, _load
    ref = R.vit_refs()
    sd, x, labels, names = ref["sd"], ref["x"], ref["labels"], ref["names"]
    fac = lambda torch_weights=None, **kw: eqv.utils.load_torch_weights(eqv.models.VisionTransformer(**kw), torch_weights)
    net = _load(fac, sd, img_size=32, patch_size=8, embed_dim=64, depth=2, num_heads=2, num_classes=R.VIT_CLASSES)
    keys = _keys(R.VIT_B)

    def loss_fn(dtype):
        @eqv.filter_value_and_grad(matmul_dtype=dtype)
        def compute_loss(model, xx, yy):
            out = eqv.vmap(model, axis_name="batch")(xx, key=keys)
            return eqv.optim.softmax_cross_entropy(out, eqv.optim.one_hot(yy, R.VIT_CLASSES)).mean()
        return compute_loss

    def grads_of(dtype):
        loss, grads = loss_fn(dtype)(net, x, labels)
        got = eqv.utils.state_dict(grads)
        got_l = [v for k, v in got.items() if "running" not in k and np.asarray(v).dtype.kind == "f"]
        assert len(got_l) == len(names)
        return loss, {n: np.asarray(v, F64) for n, v in zip(names, got_l)}

    loss_bf, g_bf = grads_of("bf16")
    loss_32, g_32 = grads_of("fp32")
    a, b = _flat(ref["a"][1], names), _flat(ref["b"][1], names)
    l2 = lambda u, v: float(np.linalg.norm(u - v) / np.linalg.norm(v))
    d_gpu_b, d_b_a, d_32_a = l2(_flat(g_bf, names), b), l2(b, a), l2(_flat(g_32, names), a)
    print(f"vit/model: loss bf16 {loss_bf:.6f} fp32 {loss_32:.6f} ref(a) {ref['a'][0]:.6f} ref(b) {ref['b'][0]:.6f} | rel L2 device-bf16 vs (b) "
          f"{d_gpu_b:.3e}, (b) vs (a) {d_b_a:.3e}, ratio {d_gpu_b / d_b_a:.4f} | device-fp32 vs (a) {d_32_a:.3e}")
    assert np.isfinite(loss_bf)
    for n in names:
        assert np.isfinite(g_bf[n]).all() and np.abs(g_bf[n]).max() > 0, f"{n}: no gradient"
    assert d_b_a > 1e-4
    assert d_gpu_b <= 0.25 * d_b_a, (d_gpu_b, d_b_a)

    # two adamw steps under "bf16": finite losses, every leaf moves
    opt = eqv.optim.adamw(learning_rate=1e-3)
    st = opt.init(eqv.filter(net, eqv.is_array))
    before = [np.array(l, copy=True) for l in eqv.tree_leaves(net) if eqv.is_array(l) and l.dtype.kind == "f"]
    m, fn = net, loss_fn("bf16")
    for _ in range(2):
        loss, grads = fn(m, x, labels)
        assert np.isfinite(loss)
        updates, st = opt.update(grads, st, eqv.filter(m, eqv.is_array))
        m = eqv.apply_updates(m, updates)
    after = [np.asarray(l) for l in eqv.tree_leaves(m) if eqv.is_array(l) and l.dtype.kind == "f"]
    assert len(before) == len(after) and all(not np.array_equal(p, q) for p, q in zip(before, after))
