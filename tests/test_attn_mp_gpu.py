"""`-m gpu`: the mixed-precision attention core (csrc/attn_mp.hip: mv_mha_mp_fwd / mv_mha_mp_bwd) through the C ABI, and the rule and the
model that use it (filter_value_and_grad(..., attn_dtype="bf16")).  References, bounds, constructions and the emulation that proves the
instruments on the CPU: tests/_attn_mp_ref.py, tests/test_attn_mp_host.py.

Every destination is sentinel-filled with a guard band behind it; the backward is handed the forward's own out and lse, as the rule
does.  Shapes (B, H, N, dh): R.SHAPES.

1. exact: select / tie / flat with a power-of-two scale -- out and lse within 2^-21 relative, dQ = dK = 0 and dV the exact sums on
   select, all three gradients bit-equal to float64 on tie (N = 1 has no tie: a tie needs two keys).
2. Gaussian fp32 operands, all five outputs per element within the counted bounds, the rounding bias of out and dV alongside.
3. determinism of the backward; probs on request within its bound and without effect on any other output; refusals.
4. the rule's launches under each setting, and the vit of tests/test_linear_mp_gpu.py::test_vit_model with only attn_dtype="bf16".

Measured on an MI355X (every exact case was exact), worst |got - ref| / bound per entry over the eight Gaussian cases:
    out 0.912, lse 0.040, probs 0.030, dQ 0.919, dK 0.909, dV 0.918, all at N = 5 (the bound is led by the bf16 half-ulps of P and dS, a
    worst case that a sum of five terms nearly reaches); at N = 197: out 0.320, lse 0.017, probs 0.011, dQ 0.467, dK 0.492, dV 0.335.
    rounding bias of out / dV at most 0.027 output ulps (limit 0.05)
    model  relative L2 of the device under attn_dtype="bf16" against (b) 3.676e-06; (b) against (a) 6.580e-04: ratio 0.0056 (allowed 0.25);
           the device's fp32 path against (a) 1.465e-07
"""
import numpy as np
import pytest
import torch

from eqxvision_amd import _lib
from tests import _attn_mp_ref as R
from tests import _linear_mp_ref as LR
from tests import _strict as S
from tests._strict_gpu import _guard_ok, _need_gpu, _out_guarded, _p, _stream  # noqa: F401  (_need_gpu: the module fixture)

pytestmark = pytest.mark.gpu
F64 = np.float64
IDS = [R.shape_id(s) for s in R.SHAPES]


def _f(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def _launch(c, want_probs=False, repeat_bwd=False):
    """Forward then backward of a case on sentinel-filled, guarded destinations -> dict of float64 group arrays (+ "kernels")."""
    B, H = c["B"], c["H"]
    N, dh = c["q"].shape[1:]
    D = H * dh
    qkv = _f(R.mha_pack(c["q"], c["k"], c["v"], B, H))
    dout = _f(c["dout"].reshape(B, H, N, dh).transpose(0, 2, 1, 3).reshape(B, N, D))
    bufs = {t: _out_guarded(s, "fp32") for t, s in (("out", (B, N, D)), ("lse", (B, H, N)), ("dqkv", (B, N, 3 * D)))}
    if want_probs:
        bufs["probs"] = _out_guarded((B, H, N, N), "fp32")
    y = {t: v[1] for t, v in bufs.items()}
    sc = float(c["scale"])
    _lib.call("mv_mha_mp_fwd", _p(qkv), _p(y["out"]), _p(y["lse"]), _p(y.get("probs")), B, N, H, dh, sc, _stream())
    kf = _lib.last_kernel()
    _lib.call("mv_mha_mp_bwd", _p(qkv), _p(y["out"]), _p(dout), _p(y["lse"]), _p(y["dqkv"]), B, N, H, dh, sc, _stream())
    kb = _lib.last_kernel()
    torch.cuda.synchronize()
    for t, (buf, _) in bufs.items():
        assert _guard_ok(buf), f"guard band behind {t} touched"
        assert not bool((bufs[t][1] == S.SENTINEL).all().item()), f"{t} was not written"
    d = y["dqkv"].cpu().numpy().astype(F64)
    got = {"out": R.mha_groups(y["out"].cpu().numpy().astype(F64), H), "lse": y["lse"].cpu().numpy().astype(F64).reshape(B * H, N),
           "dq": R.mha_groups(d[:, :, :D], H), "dk": R.mha_groups(d[:, :, D:2 * D], H), "dv": R.mha_groups(d[:, :, 2 * D:], H),
           "kernels": (kf, kb), "raw": {t: v.clone() for t, v in y.items()}}
    if want_probs:
        got["probs"] = y["probs"].cpu().numpy().astype(F64).reshape(B * H, N, N)
    if repeat_bwd:
        buf2, d2 = _out_guarded((B, N, 3 * D), "fp32")
        _lib.call("mv_mha_mp_bwd", _p(qkv), _p(y["out"]), _p(dout), _p(y["lse"]), _p(d2), B, N, H, dh, sc, _stream())
        torch.cuda.synchronize()
        assert _guard_ok(buf2)
        got["dqkv2"] = d2
    return got


def _kernels_ok(got, dh):
    assert got["kernels"] == (f"mha_mp_fwd_dh{dh}", f"mha_mp_bwd_dh{dh}"), got["kernels"]


# ================================================================================================ 1. exact
EXACT = [(s, kind) for s in R.SHAPES for kind in ("select", "tie", "flat") if kind != "tie" or R.has_tie(s)]


@pytest.mark.parametrize("shape,kind", EXACT, ids=[f"{R.shape_id(s)}-{k}" for s, k in EXACT])
def test_exact(shape, kind):
    p = R.exact_case(kind, shape)
    R.prove_exact_case(p)
    got = _launch(p)
    _kernels_ok(got, shape[3])
    fwd = R.check_exact_fwd(got, p)
    print(f"attn_mp/{kind}/{R.shape_id(shape)}: fwd {({t: v.get('worst') for t, v in fwd.items() if isinstance(v, dict)})}")
    assert fwd["ok"], fwd
    if kind != "flat":
        bwd = R.check_exact_bwd(got, p)
        print(f"attn_mp/{kind}/{R.shape_id(shape)}: bwd exact {({t: v['ok'] for t, v in bwd.items() if isinstance(v, dict)})}")
        assert bwd["ok"], bwd


# ================================================================================================ 2. Gaussian, per element
@pytest.mark.parametrize("shape", R.SHAPES, ids=IDS)
def test_gauss(shape):
    c = R.gauss_case(shape)
    got = _launch(c, want_probs=True)
    _kernels_ok(got, shape[3])
    info = R.check_gauss(got, c, probs=got["probs"])
    print(f"attn_mp/gauss/{R.shape_id(R.gauss_shape(shape))}: worst error/bound {R.worst(info)} | bias out "
          f"{info.get('out_bias', {}).get('bias')} dv {info.get('dv_bias', {}).get('bias')}")
    assert info["ok"], info


# ================================================================================================ 3. determinism, probs, refusals
@pytest.mark.parametrize("shape", [(2, 2, 65, 64), (1, 1, 197, 64)], ids=["2x2x65x64", "1x1x197x64"])
def test_bwd_is_deterministic_and_probs_change_nothing(shape):
    c = R.gauss_case(shape)
    a = _launch(c, repeat_bwd=True)
    assert torch.equal(a["raw"]["dqkv"], a["dqkv2"]), "two backward launches differ"
    b = _launch(c, want_probs=True)
    for t in ("out", "lse", "dqkv"):
        assert torch.equal(a["raw"][t], b["raw"][t]), f"{t} depends on whether probs was requested"


@pytest.mark.parametrize("what", ("N257", "N0", "dh48", "null"))
def test_refusals(what):
    B, H, N, dh = 1, 1, 17, 32
    if what == "N257":
        N = 257
    elif what == "N0":
        N = 0
    elif what == "dh48":
        dh = 48
    n = max(N, 1)
    qkv = torch.zeros((B, n, 3 * H * dh), device="cuda")
    out, lse, dqkv = (torch.full(s, S.SENTINEL, device="cuda") for s in ((B, n, H * dh), (B, H, n), (B, n, 3 * H * dh)))
    lib = _lib.load()
    assert bool(lib.mv_mha_mp_supported(N, dh)) == (what == "null")
    qp = None if what == "null" else _p(qkv)
    rc = lib.mv_mha_mp_fwd(qp, _p(out), _p(lse), None, B, N, H, dh, 0.25, _stream())
    assert rc < 0 and lib.mv_last_error()
    rc = lib.mv_mha_mp_bwd(qp, _p(out), _p(out), _p(lse), _p(dqkv), B, N, H, dh, 0.25, _stream())
    assert rc < 0 and lib.mv_last_error()
    if what == "null":
        assert lib.mv_mha_mp_bwd(_p(qkv), _p(out), _p(out), _p(lse), None, B, N, H, dh, 0.25, _stream()) < 0
    torch.cuda.synchronize()
    for t in (out, lse, dqkv):
        assert bool((t == S.SENTINEL).all().item()), f"{what}: a refused call wrote its destination"


# ================================================================================================ 4. the rule and a model
def _vit():
    import eqxvision_amd as eqv
    from tests._model_cases import _keys, _load
    ref = LR.vit_refs()
    fac = lambda torch_weights=None, **kw: eqv.utils.load_torch_weights(eqv.models.VisionTransformer(**kw), torch_weights)
    net = _load(fac, ref["sd"], img_size=32, patch_size=8, embed_dim=64, depth=2, num_heads=2, num_classes=LR.VIT_CLASSES)
    keys = _keys(LR.VIT_B)

    def loss_fn(**kw):
        @eqv.filter_value_and_grad(**kw)
        def compute_loss(model, xx, yy):
            out = eqv.vmap(model, axis_name="batch")(xx, key=keys)
            return eqv.optim.softmax_cross_entropy(out, eqv.optim.one_hot(yy, LR.VIT_CLASSES)).mean()
        return compute_loss

    def grads_of(**kw):
        loss, grads = loss_fn(**kw)(net, ref["x"], ref["labels"])
        got = eqv.utils.state_dict(grads)
        got_l = [v for k, v in got.items() if "running" not in k and np.asarray(v).dtype.kind == "f"]
        assert len(got_l) == len(ref["names"])
        return loss, {n: np.asarray(v, F64) for n, v in zip(ref["names"], got_l)}
    return ref, net, loss_fn, grads_of


def _record(monkeypatch):
    calls = []
    orig = _lib.call

    def rec(name, *args):
        calls.append((name, args))
        return orig(name, *args)
    monkeypatch.setattr(_lib, "call", rec)
    return calls


def test_rule_launches(monkeypatch):
    ref, net, loss_fn, grads_of = _vit()
    calls = _record(monkeypatch)
    loss, _ = grads_of(attn_dtype="bf16")
    names = [n for n, _ in calls]
    assert names.count("mv_mha_mp_fwd") == 2 and names.count("mv_mha_mp_bwd") == 2, names
    assert "mv_mha_bwd_f32" not in names and "mv_mha_fwd" not in names and "mv_linear_mp_fwd" not in names
    assert all(a[3] is None for n, a in calls if n == "mv_mha_mp_fwd"), "probs allocated although need_probs is false"
    assert np.isfinite(loss)
    del calls[:]
    _, g1 = grads_of()
    names = [n for n, _ in calls]
    assert names.count("mv_mha_fwd") == 2 and names.count("mv_mha_bwd_f32") == 2 and not any(n.startswith("mv_mha_mp") for n in names)
    _, g2 = grads_of()
    assert all(np.array_equal(g1[n], g2[n]) for n in g1), "the default path is not reproducible"
    del calls[:]
    loss3, g3 = grads_of(attn_dtype="bf16", matmul_dtype="bf16", conv_dtype="bf16")
    names = [n for n, _ in calls]
    assert "mv_mha_mp_fwd" in names and "mv_linear_mp_fwd" in names and "mv_mha_bwd_f32" not in names
    assert np.isfinite(loss3) and all(np.isfinite(v).all() for v in g3.values())


def _vit_ref_b():
    """float64 with the attention core rounding as the contract says (r on q, k, v, dout, P and dS; delta and the sums un-rounded): the
    oracle's block with its attention replaced, for the duration of the call, by an autograd Function."""
    from oracle import torch_grad as TG
    from oracle import torch_ref as TR
    import torch.nn.functional as F
    ref = LR.vit_refs()

    def r(t):
        return torch.from_numpy(LR.rne_bf16(t.detach().to(torch.float32).numpy()).astype(F64))

    class Core(torch.autograd.Function):
        @staticmethod
        def forward(ctx, q, k, v, scale):
            qr, kr, vr = r(q), r(k), r(v)
            L = qr @ kr.transpose(-2, -1) * scale
            m = L.max(-1, keepdim=True).values
            pe = torch.exp(L - m)
            Z = pe.sum(-1, keepdim=True)
            out = (r(pe) @ vr) / Z
            ctx.save_for_backward(qr, kr, vr, out, m + torch.log(Z))
            ctx.scale = scale
            return out

        @staticmethod
        def backward(ctx, g):
            qr, kr, vr, out, lse = ctx.saved_tensors
            gr = r(g)
            p = torch.exp(qr @ kr.transpose(-2, -1) * ctx.scale - lse)
            delta = (g.to(torch.float32).to(torch.float64) * out.to(torch.float32).to(torch.float64)).sum(-1, keepdim=True)
            ds = ctx.scale * p * (gr @ vr.transpose(-2, -1) - delta)
            return r(ds) @ kr, r(ds).transpose(-2, -1) @ qr, r(p).transpose(-2, -1) @ gr, None

    def block(sd, x, p, H, return_attention=False):
        B, N, C = x.shape
        y = F.layer_norm(x, (C,), sd[p + ".norm1.weight"], sd[p + ".norm1.bias"], 1e-5)
        qkv = F.linear(y, sd[p + ".attn.qkv.weight"], sd.get(p + ".attn.qkv.bias")).reshape(B, N, 3, H, C // H).permute(2, 0, 3, 1, 4)
        y = Core.apply(qkv[0], qkv[1], qkv[2], (C // H) ** -0.5).transpose(1, 2).reshape(B, N, C)
        x = x + F.linear(y, sd[p + ".attn.proj.weight"], sd[p + ".attn.proj.bias"])
        y = F.layer_norm(x, (C,), sd[p + ".norm2.weight"], sd[p + ".norm2.bias"], 1e-5)
        y = F.gelu(F.linear(y, sd[p + ".mlp.fc1.weight"], sd[p + ".mlp.fc1.bias"]), approximate="tanh")
        return x + F.linear(y, sd[p + ".mlp.fc2.weight"], sd[p + ".mlp.fc2.bias"])

    saved = TR._vit_block
    TR._vit_block = block
    try:
        return TG.vit(ref["sd"], ref["x"], ref["labels"], 8, 2, 2, dtype=torch.float64)
    finally:
        TR._vit_block = saved


def test_vit_model():
    """vit 32 x 32, patch 8, width 64, depth 2, 2 heads, B = 2 (N = 17, dh = 32), only attn_dtype="bf16".  (a) float64, (b) float64 with
    the attention core rounding as specified, (c) the device's fp32 path.  The device under "bf16" may differ from (b) only by fp32
    summation order and the few values that this pushes across a bf16 rounding boundary: its relative L2 distance to (b) over all
    parameter gradients is at most a quarter of the distance of (b) to (a); (b) - (a) is well above (c) - (a): the option is live."""
    import eqxvision_amd as eqv
    ref, net, loss_fn, grads_of = _vit()
    names = ref["names"]
    flat = lambda g: np.concatenate([np.asarray(g[n], F64).reshape(-1) for n in names])
    loss_b, gb = _vit_ref_b()
    loss_bf, g_bf = grads_of(attn_dtype="bf16")
    loss_32, g_32 = grads_of()
    a, b = flat(ref["a"][1]), flat(gb)
    l2 = lambda u, v: float(np.linalg.norm(u - v) / np.linalg.norm(v))
    d_gpu_b, d_b_a, d_32_a = l2(flat(g_bf), b), l2(b, a), l2(flat(g_32), a)
    print(f"vit/attn_mp: loss bf16 {loss_bf:.6f} fp32 {loss_32:.6f} ref(a) {ref['a'][0]:.6f} ref(b) {loss_b:.6f} | rel L2 device-bf16 vs (b) "
          f"{d_gpu_b:.3e}, (b) vs (a) {d_b_a:.3e}, ratio {d_gpu_b / d_b_a:.4f} | device-fp32 vs (a) {d_32_a:.3e}")
    assert np.isfinite(loss_bf)
    for n in names:
        assert np.isfinite(g_bf[n]).all() and np.abs(g_bf[n]).max() > 0, f"{n}: no gradient"
    assert d_b_a >= 100 * d_32_a, (d_b_a, d_32_a)                    # the rounding is two orders above the fp32 path's own error
    assert d_gpu_b <= 0.25 * d_b_a, (d_gpu_b, d_b_a)

    opt = eqv.optim.adamw(learning_rate=1e-3)
    st = opt.init(eqv.filter(net, eqv.is_array))
    m, fn = net, loss_fn(attn_dtype="bf16")
    for _ in range(2):
        loss, grads = fn(m, ref["x"], ref["labels"])
        assert np.isfinite(loss)
        updates, st = opt.update(grads, st, eqv.filter(m, eqv.is_array))
        m = eqv.apply_updates(m, updates)
