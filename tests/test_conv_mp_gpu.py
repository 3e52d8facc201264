"""`-m gpu`: the mixed-precision Conv2d kernels (csrc/conv_mp.hip: mv_conv2d_mp_fwd / _dgrad / _wgrad) and the rule that uses them
(filter_value_and_grad(..., conv_dtype="bf16")).  References, case generators, split arithmetic and the model emulation:
tests/_conv_mp_ref.py; the CPU proof that the cases see a wrong rounding, fp32 products, a rounded bias, a missing stride test, swapped
taps, an ignored dilation and a dropped ragged chunk: tests/test_conv_mp_host.py.

Every destination is sentinel-filled with a guard behind it, the serving kernel is asserted (`_lib.last_kernel()`), references are
float64 on the bf16-rounded operands.

1. exact, integers in [-2, 2], the nine shapes of R.SHAPES, three entries, the forward with and without bias.
2. exact with the rounding visible: operands k 2^-10 with every tie class, reduction 16, a bias that is no bf16 value.
3. wgrad under every scratch regime (no offer, ample, room for 2.5 parts, room for 1.5) on the split shape and on shape 8: bit-equal to
   the reference and to each other, the kernel name per regime, bytes [0, 4096) of the offer left zero.
4. Gaussian operands within S.elem_bound(ref, mag, kred, "fp32"), kred = R S C / K R S / P: holds for any summation order.
5. the rule: g_conv2d under "bf16" (y, dx, dW, db each to its own bound; the launch list; pointwise stride 1 -> mv_linear_mp_*;
   depthwise, frozen weight, input off the tape, the default).
6. a model: resnet18 (32 x 32) against a float64 emulation that rounds x, w and the incoming gradient of every convolution.

Measured on an MI355X, worst |got - ref| / bound per entry over the shapes of case 4 (every exact case was bit-equal, under every
scratch regime):
    fwd    0.014 (shape 2, C = 3)
    dgrad  0.005 (shape 7, the strided pointwise)
    wgrad  0.039 (shape 9, P = 9); 0.002 at 2 x 14 x 14 x 256 -> 256
    rule   y 0.003, dx 0.002, dW 0.011, db 0.029; pointwise (as a Linear) y 0.022, dx 0.009, dW 0.007
    model  relative L2 of the device under "bf16" against (b) 8.288e-04; (b) against (a) 2.380e-02: ratio 0.0348 (allowed 0.25); the
           device's fp32 path against (a) 2.385e-07
"""
import contextlib
import types

import numpy as np
import pytest
import torch

from eqxvision_amd import _lib
from tests import _conv_mp_ref as R
from tests import _strict as S
from tests._strict_gpu import _Flags, _need_gpu, _p, _stream  # noqa: F401  (_need_gpu: the module fixture)
from tests.test_strict_bwd_gpu import AMPLE, SYNC, _f, _Scratch
from tests.test_strict_mem_gpu import _judge, _run

pytestmark = pytest.mark.gpu
F64 = np.float64
KERNEL = {"fwd": "conv_mp_fwd_bf16", "dgrad": "conv_mp_dgrad_bf16", "wgrad": "conv_mp_wgrad_bf16"}
SPLIT = "conv_mp_wgrad_split_bf16"
IDS = [g.tag for g in R.SHAPES]


def _launch(entry, g, x, w, dy, bias=None, offer=None):
    """One launch on a sentinel-filled, guarded destination -> (values as float64, kernel name)."""
    xd, wd, gd = (None if a is None else _f(a) for a in (x, w, dy))
    bd = None if bias is None else _f(bias)
    tail = R.args_of(g) + (_stream(),)
    with _Scratch(offer):
        if entry == "fwd":
            return _run("mv_conv2d_mp_fwd", lambda y: (_p(xd), _p(wd), _p(bd), y) + tail, R.out_shape(entry, g), "fp32")
        if entry == "dgrad":
            return _run("mv_conv2d_mp_dgrad", lambda y: (_p(gd), _p(wd), y) + tail, R.out_shape(entry, g), "fp32")
        return _run("mv_conv2d_mp_wgrad", lambda y: (_p(xd), _p(gd), y) + tail, R.out_shape(entry, g), "fp32")


# ================================================================================================ 1. exact, integers
@pytest.mark.parametrize("entry", R.ENTRIES)
@pytest.mark.parametrize("g", R.SHAPES, ids=IDS)
def test_exact_int(g, entry):
    x, w, dy, bias = R.int_case(g)
    for b in ((None, bias) if entry == "fwd" else (None,)):
        ref, mag = R.product_ref(entry, g, x, w, dy, b)
        S.prove_exact(f"conv_mp/{entry}/{g.tag}", ref, mag, R.weights_of(entry, g, x, w, dy), out="fp32")
        got, kern = _launch(entry, g, x, w, dy, b)
        _judge(f"conv_mp/{entry}/int/{g.tag}/{'bias' if b is not None else 'nobias'}", kern, KERNEL[entry], got, ref, "fp32")
        assert np.array_equal(got, ref)


# ================================================================================================ 2. exact, rounding visible
@pytest.mark.parametrize("entry", R.ENTRIES)
def test_exact_rounding(entry):
    g = R.ROUND_SHAPES[entry]
    x, w, dy, bias = R.round_case(entry)
    ref, mag = R.product_ref(entry, g, x, w, dy, bias)
    R.prove_round_case(entry, g, ref, mag, x, w, dy, bias)
    got, kern = _launch(entry, g, x, w, dy, bias if entry == "fwd" else None)
    _judge(f"conv_mp/{entry}/round/{g.tag}", kern, KERNEL[entry], got, ref, "fp32")
    assert np.array_equal(got, ref)


# ================================================================================================ 3. wgrad, scratch regimes
def _regimes(out_elems):
    return [("no_offer", None), ("ample", AMPLE), ("fit2", SYNC + int(2.5 * out_elems * 4)), ("fit1", SYNC + int(1.5 * out_elems * 4))]


@pytest.mark.parametrize("g", [R.SPLIT_SHAPE, R.SHAPES[7]], ids=["split_shape", "shape8"])
def test_wgrad_scratch_regimes(g):
    x, w, dy, _ = R.int_case(g)
    ref, mag = R.product_ref("wgrad", g, x, w, dy)
    S.prove_exact(f"conv_mp/wgrad/{g.tag}", ref, mag, R.weights_of("wgrad", g, x, w, dy), out="fp32")
    results = []
    for name, offer in _regimes(g.out_elems):
        parts = R.wgrad_split(g, offer)[1]
        got, kern = _launch("wgrad", g, x, w, dy, offer=offer)              # (_Scratch asserts bytes [0, 4096) of the offer are zero)
        _judge(f"conv_mp/wgrad/{g.tag}/{name}/parts{parts}", kern, SPLIT if parts > 1 else KERNEL["wgrad"], got, ref, "fp32")
        results.append(got)
    for r in results:
        assert np.array_equal(r, ref) and np.array_equal(r, results[0])


# ================================================================================================ 4. bounded, Gaussian
BOUND_IDS = [g.tag for g in R.BOUND_SHAPES]


@pytest.mark.parametrize("entry", R.ENTRIES)
@pytest.mark.parametrize("g", R.BOUND_SHAPES, ids=BOUND_IDS)
def test_bounded_gauss(g, entry):
    x, w, dy, bias = R.gauss_case(g)
    b = bias if entry == "fwd" else None
    ref, mag = R.product_ref(entry, g, x, w, dy, b)
    bound = S.elem_bound(ref, mag, R.kred_of(entry, g), "fp32")
    offers = (None, AMPLE) if entry == "wgrad" else (None,)
    for offer in offers:
        parts = R.wgrad_split(g, offer)[1] if entry == "wgrad" else 1
        got, kern = _launch(entry, g, x, w, dy, b, offer=offer)
        _judge(f"conv_mp/{entry}/gauss/{g.tag}/parts{parts}", kern, SPLIT if parts > 1 else KERNEL[entry], got, ref, "fp32", bound=bound)


# ================================================================================================ 5. the rule
MP_ENTRIES = ("mv_conv2d_mp_fwd", "mv_conv2d_mp_dgrad", "mv_conv2d_mp_wgrad")
LIN_ENTRIES = ("mv_linear_mp_fwd", "mv_linear_mp_dgrad", "mv_linear_mp_wgrad")
FP32_ENTRIES = ("mv_conv2d_nhwc_fwd", "mv_conv2d_dgrad_nhwc_f32", "mv_conv2d_wgrad_nhwc_f32")


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
    """A parameter leaf [B, H, W, C] as a map on the tape: its gradient is the gradient that reaches the activation."""
    from eqxvision_amd import grad
    from eqxvision_amd._act import Act
    a = Act(grad._leaf_dev(leaf), "map", True)

    def backward(g):
        grad._acc_param(leaf, g)
        return ()
    a.node = grad.Node([], backward)
    return a


def _off_tape(leaf):
    from eqxvision_amd._act import Act
    return Act(_f(leaf), "map", True)


def _rule(g, use_bias=True, extras=True, groups=1, freeze_weight=False, x_on_tape=True, **kw):
    """One nn.Conv2d of geometry `g` on a [N, H, W, C] map (+ residual and relu with `extras`) under filter_value_and_grad(**kw), the loss
    <y, G0>.  Returns (model, G0 as NHWK, y as NHWK, grads as float64 arrays, the entries called)."""
    import eqxvision_amd as eqv
    from eqxvision_amd import nn, ops
    from tests._rule_grad import linear_loss
    rng = S.rng_of(37)
    conv = nn.Conv2d(g.C, g.K, (g.R, g.S), (g.sh, g.sw), (g.ph, g.pw), (g.dh, g.dw), groups, use_bias=use_bias, key=eqv.random.PRNGKey(1))
    cg = g.C // groups
    conv.weight = (rng.standard_normal((g.K, cg, g.R, g.S)) / np.sqrt(cg * g.R * g.S)).astype(np.float32)
    if use_bias:
        conv.bias = (0.1 * rng.standard_normal((g.K, 1, 1))).astype(np.float32)
    model = {"x0": rng.standard_normal((g.N, g.H, g.W, g.C)).astype(np.float32), "conv": conv}
    if extras:
        model["r0"] = rng.standard_normal((g.N, g.Ho, g.Wo, g.K)).astype(np.float32)
    G0 = rng.standard_normal((g.N, g.Ho, g.Wo, g.K)).astype(np.float32)
    seen = {}
    spec = None
    if freeze_weight:
        spec = {k: True for k in model}
        spec["conv"] = eqv.tree_map(lambda l: l is not conv.weight, conv)

    @eqv.filter_value_and_grad(arg=spec, **kw)
    def fn(m):
        xa = _leaf_act(m["x0"]) if x_on_tape else _off_tape(m["x0"])
        y = ops.conv2d(xa, m["conv"], None, "relu", _leaf_act(m["r0"])) if extras else ops.conv2d(xa, m["conv"])
        seen["y"] = y.t.detach().cpu().numpy().astype(F64)
        return linear_loss(types.SimpleNamespace(act=y), G0.transpose(0, 3, 1, 2))

    with _calls() as names:
        _, grads = fn(model)
    out = {"x0": np.asarray(grads["x0"], F64), "w": None if grads["conv"].weight is None else np.asarray(grads["conv"].weight, F64)}
    if use_bias:
        out["b"] = np.asarray(grads["conv"].bias, F64).reshape(-1)
    if extras:
        out["r0"] = np.asarray(grads["r0"], F64)
    return model, G0, seen["y"], out, names


def _within(tag, got, ref, bound):
    i = S.check_bound(got, ref, None, 0, "fp32", bound=bound)
    print(f"{tag}: worst |got-ref|/bound {i.get('worst', float('nan')):.3f} over {i.get('n')} elements, violations {i.get('nviol')}")
    assert i["ok"], (tag, i)


RULE_GEOM = S.ConvGeom(2, 9, 7, 16, 24, (3, 3), 2, 1, 1, 1)


def test_rule():
    """One Conv2d on a [2, 9, 7, 16] map, 3 x 3, stride 2, with bias + residual + relu.  g2 = G0 [z > 0] is computed by mv_act_bwd_f32 from
    the DEVICE's z; it is the residual's gradient, and must be G0 or 0 element by element and agree with the float64 mask wherever z is not
    within its own bound of zero.  dx, dW and db are referred to the device's g2, so that each product is held to the bound that follows
    from its own arithmetic."""
    g = RULE_GEOM
    model, G0, y, got, names = _rule(g, conv_dtype="bf16")
    x, w_oihw, bias = model["x0"], model["conv"].weight, model["conv"].bias.reshape(-1)
    w = np.ascontiguousarray(w_oihw.transpose(0, 2, 3, 1))                   # KRSC
    r = R.rule_ref(g, x, w, bias, model["r0"], G0)
    assert [names.count(n) for n in MP_ENTRIES] == [1, 1, 1]
    assert not any(n in names for n in FP32_ENTRIES + LIN_ENTRIES)
    assert names[names.index("mv_conv2d_mp_wgrad") - 1] == "mv_set_scratch"
    yref, zmag = r["y"]
    zbound = S.elem_bound(r["z"], zmag, R.kred_of("fwd", g), "fp32")
    _within("rule/y", y, yref, zbound)                                        # relu is 1-Lipschitz and exact
    g2 = got["r0"].astype(np.float32)
    G32 = G0.astype(np.float32)
    assert ((g2 == G32) | (g2 == 0)).all()
    sure = np.abs(r["z"]) > zbound
    assert np.array_equal(g2[sure].astype(F64), r["g2"][sure]) and sure.mean() > 0.99
    dx, dxmag = R.product_ref("dgrad", g, w=w, dy=g2)
    _within("rule/dx", got["x0"], dx, S.elem_bound(dx, dxmag, R.kred_of("dgrad", g), "fp32"))
    dw, dwmag = R.product_ref("wgrad", g, x=x, dy=g2)
    _within("rule/dW", got["w"].transpose(0, 2, 3, 1), dw, S.elem_bound(dw, dwmag, g.P, "fp32"))
    g64 = g2.astype(F64).reshape(-1, g.K)
    db, dbmag = g64.sum(0), np.abs(g64).sum(0)
    _within("rule/db", got["b"], db, S.ops_bound(db, dbmag, S.colsum_n_ops(g.P, 1), "fp32"))


def test_rule_pointwise_is_a_linear():
    """1 x 1, stride 1, no padding: the three products run as mv_linear_mp_* on the [N H W, C] rows, no conv entry is launched, and the
    values are those of the conv references (dW[K, C] is the leaf's (K, C, 1, 1) memory)."""
    g = S.ConvGeom(2, 5, 7, 24, 40, (1, 1), 1, 0, 1, 1)
    model, G0, y, got, names = _rule(g, extras=False, conv_dtype="bf16")
    assert [names.count(n) for n in LIN_ENTRIES] == [1, 1, 1]
    assert not any(n in names for n in MP_ENTRIES + FP32_ENTRIES) and "mv_nhwc_to_nchw" not in names
    assert names[names.index("mv_linear_mp_wgrad") - 1] == "mv_set_scratch"
    x, bias = model["x0"], model["conv"].bias.reshape(-1)
    w = np.ascontiguousarray(model["conv"].weight.transpose(0, 2, 3, 1))
    for tag, have, (ref, mag), kred in (("y", y, R.product_ref("fwd", g, x, w, None, bias), g.C),
                                        ("dx", got["x0"], R.product_ref("dgrad", g, w=w, dy=G0), g.K),
                                        ("dW", got["w"].transpose(0, 2, 3, 1), R.product_ref("wgrad", g, x=x, dy=G0), g.P)):
        _within(f"rule/pointwise/{tag}", have, ref, S.elem_bound(ref, mag, kred, "fp32"))


def test_rule_depthwise_is_the_default_path():
    """groups > 1 under "bf16": launch for launch and bit for bit the default."""
    g = S.ConvGeom(2, 7, 7, 12, 12, (3, 3), 2, 1, 1, 1)
    a = _rule(g, groups=12, conv_dtype="bf16")
    b = _rule(g, groups=12)
    assert a[4] == b[4] and not any(n in a[4] for n in MP_ENTRIES + LIN_ENTRIES) and [a[4].count(n) for n in FP32_ENTRIES] == [1, 1, 1]
    assert np.array_equal(a[2], b[2]) and all(np.array_equal(a[3][k], b[3][k]) for k in a[3])


def test_rule_frozen_weight_launches_no_wgrad():
    model, G0, y, got, names = _rule(RULE_GEOM, freeze_weight=True, conv_dtype="bf16")
    assert "mv_conv2d_mp_wgrad" not in names and names.count("mv_conv2d_mp_dgrad") == 1 and names.count("mv_conv2d_mp_fwd") == 1
    assert got["w"] is None and np.abs(got["x0"]).max() > 0 and np.abs(got["b"]).max() > 0


def test_rule_input_off_the_tape_launches_no_dgrad():
    model, G0, y, got, names = _rule(RULE_GEOM, x_on_tape=False, conv_dtype="bf16")
    assert "mv_conv2d_mp_dgrad" not in names and names.count("mv_conv2d_mp_wgrad") == 1 and names.count("mv_conv2d_mp_fwd") == 1
    assert np.abs(got["w"]).max() > 0 and not np.abs(got["x0"]).any()


def test_default_is_fp32_path():
    """No keyword, and matmul_dtype="bf16" alone: the launches of the default path (one fp32 forward, dgrad and wgrad; no bf16 entry)."""
    base = _rule(RULE_GEOM)
    for kw in ({}, {"conv_dtype": "fp32"}, {"matmul_dtype": "bf16"}):
        run = _rule(RULE_GEOM, **kw)
        names = run[4]
        assert names == base[4] and not any(n in names for n in MP_ENTRIES + LIN_ENTRIES)
        assert [names.count(n) for n in FP32_ENTRIES] == [1, 1, 1] and names[names.index("mv_conv2d_wgrad_nhwc_f32") - 1] == "mv_set_scratch"
        assert np.array_equal(run[2], base[2]) and all(np.array_equal(run[3][k], base[3][k]) for k in base[3])


# ================================================================================================ 6. a model
def _flat(sd_like, names):
    return np.concatenate([np.asarray(sd_like[n], F64).reshape(-1) for n in names])


def test_resnet_model():
    """resnet18, 32 x 32, 5 classes, B = 2, inference-mode BatchNorm.  (a) float64, (b) float64 with every convolution rounding x, w and the
    incoming gradient, (c) the device's fp32 path.  The device under "bf16" may differ from (b) only by fp32 summation order, the ReLU /
    max-pool decisions and the few values that this pushes across a bf16 rounding boundary: its relative L2 distance to (b) must be at
    most a quarter of the distance of (b) to (a), the effect of the rounding itself (2.380e-02, asserted on the CPU)."""
    import eqxvision_amd as eqv
    from tests._model_cases import _keys, _load
    ref = R.resnet_refs()
    sd, x, labels, names = ref["sd"], ref["x"], ref["labels"], ref["names"]
    net = _load(eqv.models.resnet18, sd, num_classes=R.RESNET_CLASSES)
    keys = _keys(R.RESNET_B)

    def loss_fn(dtype):
        @eqv.filter_value_and_grad(conv_dtype=dtype)
        def compute_loss(model, xx, yy):
            out = eqv.vmap(model, axis_name="batch")(xx, key=keys)
            return eqv.optim.softmax_cross_entropy(out, eqv.optim.one_hot(yy, R.RESNET_CLASSES)).mean()
        return compute_loss

    def grads_of(dtype):
        with _calls() as called:
            loss, grads = loss_fn(dtype)(net, x, labels)
        got = eqv.utils.state_dict(grads)
        got_l = [v for k, v in got.items() if "running" not in k and np.asarray(v).dtype.kind == "f"]
        assert len(got_l) == len(names)
        return loss, {n: np.asarray(v, F64) for n, v in zip(names, got_l)}, called

    loss_bf, g_bf, called_bf = grads_of("bf16")
    loss_32, g_32, called_32 = grads_of("fp32")
    assert called_bf.count("mv_conv2d_mp_fwd") > 10 and not any(n in called_32 for n in MP_ENTRIES + LIN_ENTRIES)
    a, b = _flat(ref["a"][1], names), _flat(ref["b"][1], names)
    l2 = lambda u, v: float(np.linalg.norm(u - v) / np.linalg.norm(v))
    d_gpu_b, d_b_a, d_32_a = l2(_flat(g_bf, names), b), l2(b, a), l2(_flat(g_32, names), a)
    print(f"resnet18/model: loss bf16 {loss_bf:.6f} fp32 {loss_32:.6f} ref(a) {ref['a'][0]:.6f} ref(b) {ref['b'][0]:.6f} | rel L2 device-bf16 "
          f"vs (b) {d_gpu_b:.3e}, (b) vs (a) {d_b_a:.3e}, ratio {d_gpu_b / d_b_a:.4f} | device-fp32 vs (a) {d_32_a:.3e}")
    assert np.isfinite(loss_bf)
    for n in names:
        assert np.isfinite(g_bf[n]).all() and np.abs(g_bf[n]).max() > 0, f"{n}: no gradient"
    assert d_b_a > 1e-4
    assert d_gpu_b <= 0.25 * d_b_a, (d_gpu_b, d_b_a)

    # two adamw steps under "bf16": finite losses, every leaf moves
    opt = eqv.optim.adamw(learning_rate=1e-3)
    st = opt.init(eqv.filter(net, eqv.is_array))
    moving = lambda m: [np.array(np.asarray(v), copy=True) for k, v in eqv.utils.state_dict(m).items()
                        if "running" not in k and np.asarray(v).dtype.kind == "f"]
    before = moving(net)
    m, fn = net, loss_fn("bf16")
    for _ in range(2):
        loss, grads = fn(m, x, labels)
        assert np.isfinite(loss)
        updates, st = opt.update(grads, st, eqv.filter(m, eqv.is_array))
        m = eqv.apply_updates(m, updates)
    after = moving(m)
    assert len(before) == len(after) == len(names) and all(not np.array_equal(p, q) for p, q in zip(before, after))
