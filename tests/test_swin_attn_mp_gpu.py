"""`-m gpu`: the mixed-precision Swin window attention (csrc/swin_attn_mp.hip: mv_swin_attn_mp_fwd / mv_swin_attn_mp_bwd) through the C
ABI, and the rule and the model that use it (filter_value_and_grad(..., attn_dtype="bf16") on g_swin_window_attention).  References,
bounds, constructions and the emulation that proves the instruments on the CPU: tests/_swin_attn_mp_ref.py,
tests/test_swin_attn_mp_host.py.

Every destination is sentinel-filled with a guard band behind it; the backward is handed the forward's own out and lse, as the rule
does.  Shapes (B, Hf, Wf, C, heads, window, shift), R.SHAPES:
    (1, 2, 2, 32, 1, (1,1), (0,0))       a single key
    (2, 4, 6, 32, 1, (2,3), (1,1))       ragged first tile, rectangular window, both wraps
    (2, 8, 8, 64, 2, (4,4), (2,2))       n = 16
    (1, 3, 22, 32, 1, (3,11), (0,5))     n = 33, one key past a tile; the window covers the map's height: it wraps along the width only
    (1, 14, 14, 96, 3, (7,7), (3,3))     the workload's window
    (1, 14, 14, 96, 3, (7,7), (0,0))     the workload's window, unshifted
    (1, 16, 8, 128, 2, (8,8), (4,0))     n = 64, the limit; dh = 64; the window covers the map's width: it wraps along the height only
The Gaussian cases raise B until the output has 8192 elements (R.gauss_shape).  At all seven P = B nW: a workgroup walks one window.
R.WALK_SHAPES add the regime the workload runs in at a large batch, a workgroup that walks two windows with a ragged last round:
    (130, 8, 8, 32, 1, (2,2), (1,1))     2080 (image, window) pairs on P = 2048 parts
    (172, 14, 14, 96, 3, (7,7), (3,3))   688 pairs on P = 682 parts per head: the workload's window, both waves, the shift mask
They run in the exact (select / tie; flat at the small one), Gaussian and determinism / NULL groups: the re-staging of the images and
tables between windows, the forward's bias registers kept across them, lse and parts indexed by pair and by part, g added over two
windows in walk order, and bit-equality of two launches.

1. exact: select / tie / flat with a power-of-two scale and an integer bias -- out and lse within 2^-21 relative; dQ = dK = 0, dbias = 0
   and dV the exact sums on select; dQ, dK, dV bit-equal to float64 on tie, dbias within the relative error of the one inexact factor
   p (R.check_exact_bwd); the device's column sum of the parts against their float64 sum.
2. Gaussian fp32 operands, all six outputs per element within the counted bounds, the rounding bias of out and dV alongside.
3. determinism of the backward, NULL parts, every part written, refusals, a stable part count.
4. the rule's launches under each setting and with frozen tables, and a small Swin with only attn_dtype="bf16".

Measured on an MI355X (every exact case was exact; dbias on tie at most 0.928 of its bound, which is the relative error of p alone),
worst |got - ref| / bound per entry over the seven Gaussian cases:
    out 0.829, lse 0.036, dQ 0.833, dK 0.857, dV 0.896 (all at n = 6, where a sum of six terms nearly reaches the bf16 half-ulps of P and g
    that lead the bound), dbias 0.014; at the workload's window (n = 49, shifted): out 0.647, lse 0.029, dQ 0.648, dK 0.621, dV 0.750,
    dbias 0.014.  The fp32 emulation of the kernel on the CPU gives the same ratios to three digits.
    rounding bias of out / dV at most 0.030 output ulps (limit 0.05); the column sum of the parts at most 0.23 of its (P + 4) u bound
    model  relative L2 of the device under attn_dtype="bf16" against (b) 4.127e-05; (b) against (a) 3.589e-04: ratio 0.115 (allowed 0.25);
           the device's fp32 path against (a) 1.411e-07 (the margin of 100 is cleared 25 times over: the model was not widened)
"""
import numpy as np
import pytest
import torch

from eqxvision_amd import _lib
from tests import _linear_mp_ref as LR
from tests import _strict as S
from tests import _swin_attn_mp_ref as R
from tests._strict_gpu import _guard_ok, _need_gpu, _out_guarded, _p, _stream  # noqa: F401  (_need_gpu: the module fixture)

pytestmark = pytest.mark.gpu
F64 = np.float64
IDS = [R.shape_id(s) for s in R.SHAPES]


def _f(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def _geom_args(shape):
    B, Hf, Wf, C, heads, (wh, ww), (sh, sw) = shape
    return B, Hf, Wf, C, heads, wh, ww, sh, sw


def _launch(c, repeat_bwd=False, null_parts=False):
    """Forward then backward of a case on sentinel-filled, guarded destinations -> dict of float64 group arrays (+ "kernels", "raw")."""
    shape = c["shape"]
    d = R.dims(shape)
    ga = _geom_args(shape)
    B, Hf, Wf, C, heads, n = d["B"], d["Hf"], d["Wf"], d["C"], d["heads"], d["n"]
    qkv = _f(R.scatter(np.stack([c["q"], c["k"], c["v"]]), shape))
    dout = _f(R.scatter(c["dout"][None], shape))
    bias = _f(c["bias"])
    lib = _lib.load()
    Pn = lib.mv_swin_attn_mp_bwd_parts(B, Hf, Wf, heads, d["wh"], d["ww"])
    assert Pn == R.parts_of(shape) and Pn == lib.mv_swin_attn_mp_bwd_parts(B, Hf, Wf, heads, d["wh"], d["ww"])
    bufs = {t: _out_guarded(s, "fp32") for t, s in (("out", (B, Hf, Wf, C)), ("lse", (B * d["nW"], heads, n)), ("dqkv", (B, Hf, Wf, 3 * C)),
                                                    ("parts", (Pn, heads, n, n)))}
    y = {t: v[1] for t, v in bufs.items()}
    sc = float(c["scale"])
    _lib.call("mv_swin_attn_mp_fwd", _p(qkv), _p(bias), _p(y["out"]), _p(y["lse"]), *ga, sc, _stream())
    kf = _lib.last_kernel()
    _lib.call("mv_swin_attn_mp_bwd", _p(qkv), _p(bias), _p(y["out"]), _p(dout), _p(y["lse"]), _p(y["dqkv"]), _p(y["parts"]), *ga, sc, _stream())
    kb = _lib.last_kernel()
    db = torch.full((heads * n * n,), S.SENTINEL, device="cuda")
    _lib.call("mv_colsum_f32", _p(y["parts"]), None, _p(db), Pn, heads * n * n, _stream())       # as the rule sums the parts
    torch.cuda.synchronize()
    for t, (buf, _) in bufs.items():
        assert _guard_ok(buf), f"guard band behind {t} touched"
        assert not bool((y[t] == S.SENTINEL).all().item()), f"{t} was not written"
    if c["kind"] == "gauss":                                           # (an exact case may hold a true -7)
        assert not bool((y["parts"] == S.SENTINEL).any().item()), "an element of a part was not written"
    dq, dk, dv = R.gather(y["dqkv"].cpu().numpy().astype(F64), shape)
    got = {"out": R.gather(y["out"].cpu().numpy().astype(F64), shape)[0], "lse": y["lse"].cpu().numpy().astype(F64).reshape(d["G"], n),
           "dq": dq, "dk": dk, "dv": dv, "dbias": db.cpu().numpy().astype(F64).reshape(heads, n, n),
           "parts": y["parts"].cpu().numpy().astype(F64), "kernels": (kf, kb), "raw": {t: v.clone() for t, v in y.items()}}
    for extra, parts_ptr in (("2", "same"), ("null", None)):
        if (extra == "2" and not repeat_bwd) or (extra == "null" and not null_parts):
            continue
        buf2, d2 = _out_guarded((B, Hf, Wf, 3 * C), "fp32")
        bufp, p2 = _out_guarded((Pn, heads, n, n), "fp32")
        _lib.call("mv_swin_attn_mp_bwd", _p(qkv), _p(bias), _p(y["out"]), _p(dout), _p(y["lse"]), _p(d2), _p(p2) if parts_ptr else None, *ga,
                  sc, _stream())
        got["kernel_" + extra] = _lib.last_kernel()
        torch.cuda.synchronize()
        assert _guard_ok(buf2) and _guard_ok(bufp)
        got["dqkv_" + extra], got["parts_" + extra] = d2, p2
    return got


def _kernels_ok(got, dh):
    assert got["kernels"] == (f"swin_attn_mp_fwd_dh{dh}", f"swin_attn_mp_bwd_dh{dh}_dbias"), got["kernels"]


def _parts_sum_ok(got):
    """The device's column sum of the parts against the float64 sum of the same parts: P + 4 roundings of sum |part|."""
    Pn = got["parts"].shape[0]
    return S.check_bound(got["dbias"], got["parts"].sum(0), None, 0, "fp32", bound=(Pn + 4) * R.U * np.abs(got["parts"]).sum(0))


# ================================================================================================ 1. exact
EXACT = [(s, kind) for s in R.SHAPES for kind in ("select", "tie", "flat") if kind != "tie" or R.has_tie(s)]
EXACT += [(R.WALK_SHAPES[0], "select"), (R.WALK_SHAPES[0], "tie"), (R.WALK_SHAPES[0], "flat"), (R.WALK_SHAPES[1], "select"), (R.WALK_SHAPES[1], "tie")]


@pytest.mark.parametrize("shape,kind", EXACT, ids=[f"{R.shape_id(s)}-{k}" for s, k in EXACT])
def test_exact(shape, kind):
    p = R.exact_case(kind, shape)
    R.prove_exact_case(p)
    got = _launch(p)
    _kernels_ok(got, R.dims(shape)["dh"])
    fwd = R.check_exact_fwd(got, p)
    print(f"swin_attn_mp/{kind}/{R.shape_id(shape)}: fwd {({t: v.get('worst') for t, v in fwd.items() if isinstance(v, dict)})}")
    assert fwd["ok"], fwd
    if kind != "flat":
        bwd = R.check_exact_bwd(got, p)
        print(f"swin_attn_mp/{kind}/{R.shape_id(shape)}: bwd {({t: (v['ok'], v.get('worst')) for t, v in bwd.items() if isinstance(v, dict)})}")
        assert bwd["ok"], bwd
        ps = _parts_sum_ok(got)
        assert ps["ok"], ps


# ================================================================================================ 2. Gaussian, per element
@pytest.mark.parametrize("shape", R.SHAPES + R.WALK_SHAPES, ids=IDS + [R.shape_id(s) for s in R.WALK_SHAPES])
def test_gauss(shape):
    c = R.gauss_case(shape)
    got = _launch(c)
    _kernels_ok(got, R.dims(shape)["dh"])
    info = R.check_gauss(got, c)
    ps = _parts_sum_ok(got)
    print(f"swin_attn_mp/gauss/{R.shape_id(c['shape'])}: worst error/bound {R.worst(info)} | bias out "
          f"{info.get('out_bias', {}).get('bias')} dv {info.get('dv_bias', {}).get('bias')} | colsum of {got['parts'].shape[0]} parts {ps.get('worst')}")
    assert info["ok"], info
    assert ps["ok"], ps


# ================================================================================================ 3. determinism, parts, refusals
DET = [R.SHAPES[2], R.SHAPES[4], R.SHAPES[6]] + list(R.WALK_SHAPES)


@pytest.mark.parametrize("shape", DET, ids=[R.shape_id(s) for s in DET])
def test_bwd_is_deterministic_and_null_parts_change_nothing(shape):
    c = R.gauss_case(shape)
    a = _launch(c, repeat_bwd=True, null_parts=True)
    assert (R.walk_len(c["shape"]) == 2) == (shape in R.WALK_SHAPES)
    assert torch.equal(a["raw"]["dqkv"], a["dqkv_2"]) and torch.equal(a["raw"]["parts"], a["parts_2"]), "two backward launches differ"
    assert torch.equal(a["raw"]["dqkv"], a["dqkv_null"]), "dqkv depends on whether the parts were requested"
    assert bool((a["parts_null"] == S.SENTINEL).all().item()), "NULL parts, yet something was written"
    assert a["kernel_null"] == f"swin_attn_mp_bwd_dh{R.dims(shape)['dh']}"


def test_parts_count_is_stable_and_bounded():
    lib = _lib.load()
    for args, want in (((64, 56, 56, 3, 7, 7), 682), ((4096, 56, 56, 3, 7, 7), 682), ((4, 7, 7, 24, 7, 7), 4), ((1, 7, 7, 4096, 7, 7), 1)):
        assert lib.mv_swin_attn_mp_bwd_parts(*args) == want == lib.mv_swin_attn_mp_bwd_parts(*args), args
    _lib.set_flag("mha_mp_bwd_parts", 3)                                   # another kernel's switch: no flag moves this count
    try:
        assert lib.mv_swin_attn_mp_bwd_parts(64, 56, 56, 3, 7, 7) == 682
    finally:
        _lib.set_flag("mha_mp_bwd_parts", 0)


E_INVALID, E_UNSUPPORTED = -1, -2                                          # include/eqxvision_amd.h


@pytest.mark.parametrize("what", ("n65", "dh16", "misaligned", "window"))
def test_refusals(what):
    """n = 65 and dh = 16 are MV_E_UNSUPPORTED; a window that does not divide the map and a pointer that is not 16-byte aligned --
    each operand of each entry in turn -- are MV_E_INVALID.  Nothing is written by a refused call."""
    B, Hf, Wf, C, heads, wh, ww = 1, 8, 8, 32, 1, 4, 4
    if what == "n65":
        Hf, Wf, wh, ww = 5, 13, 5, 13
    elif what == "dh16":
        heads = 2
    elif what == "window":
        Hf = 6
    n, nW = wh * ww, max(1, (Hf // wh) * (Wf // ww))
    qkv = torch.zeros((B * Hf * Wf * 3 * C + 4,), device="cuda")
    bias = torch.zeros((heads * n * n + 4,), device="cuda")
    out, lse, dqkv, parts = (torch.full((k + 4,), S.SENTINEL, device="cuda") for k in (B * Hf * Wf * C, B * nW * heads * n, B * Hf * Wf * 3 * C,
                                                                                       heads * n * n))
    lib = _lib.load()
    assert bool(lib.mv_swin_attn_mp_supported(n, C // heads)) == (what in ("misaligned", "window"))
    want = E_UNSUPPORTED if what in ("n65", "dh16") else E_INVALID
    ga = (B, Hf, Wf, C, heads, wh, ww, 0, 0)
    fwd = [_p(qkv), _p(bias), _p(out), _p(lse)]
    bwd = [_p(qkv), _p(bias), _p(out), _p(out), _p(lse), _p(dqkv), _p(parts)]
    calls = []
    if what == "misaligned":                                               # 4 bytes off: still a float, no longer a float4
        for i in range(len(fwd)):
            calls.append((lib.mv_swin_attn_mp_fwd, fwd[:i] + [fwd[i] + 4] + fwd[i + 1:]))
        for i in range(len(bwd)):
            calls.append((lib.mv_swin_attn_mp_bwd, bwd[:i] + [bwd[i] + 4] + bwd[i + 1:]))
    else:
        calls += [(lib.mv_swin_attn_mp_fwd, fwd), (lib.mv_swin_attn_mp_bwd, bwd), (lib.mv_swin_attn_mp_bwd, bwd[:6] + [None])]
    for fn, ptrs in calls:
        rc = fn(*ptrs, *ga, 0.25, _stream())
        assert rc == want and lib.mv_last_error(), (what, rc, want, ptrs)
    torch.cuda.synchronize()
    for t in (out, lse, dqkv, parts):
        assert bool((t == S.SENTINEL).all().item()), f"{what}: a refused call wrote its destination"


# ================================================================================================ 4. the rule and a model
CLASSES, BATCH = 5, 2
CFG = dict(patch=(4, 4), depths=(2, 2), num_heads=(1, 2), window=(4, 4))


def _swin():
    import eqxvision_amd as eqv
    from oracle import state as ST
    from tests._model_cases import _keys, _load
    sd = ST.swin_state(1, (4, 4), 32, (2, 2), (1, 2), (4, 4), 4.0, CLASSES)
    x = ST.synthetic_images(BATCH, 32, seed=5)
    labels = np.arange(BATCH) % CLASSES
    fac = lambda torch_weights=None, **kw: eqv.utils.load_torch_weights(eqv.models.SwinTransformer(**kw), torch_weights)
    net = _load(fac, sd, patch_size=[4, 4], embed_dim=32, depths=[2, 2], num_heads=[1, 2], window_size=[4, 4], num_classes=CLASSES)
    keys = _keys(BATCH)

    def loss_fn(**kw):
        @eqv.filter_value_and_grad(**kw)
        def compute_loss(model, xx, yy):
            out = eqv.vmap(model, axis_name="batch")(xx, key=keys)
            return eqv.optim.softmax_cross_entropy(out, eqv.optim.one_hot(yy, CLASSES)).mean()
        return compute_loss

    def grads_of(names, **kw):
        loss, grads = loss_fn(**kw)(net, x, labels)
        got = eqv.utils.state_dict(grads)
        got_l = [v for k, v in got.items() if "running" not in k and v is not None and np.asarray(v).dtype.kind == "f"]
        assert len(got_l) == len(names), (len(got_l), len(names))
        return loss, {n: np.asarray(v, F64) for n, v in zip(names, got_l)}
    return sd, x, labels, net, loss_fn, grads_of


def _refs(sd, x, labels, attn=None):
    from oracle import torch_grad as TG
    from oracle import torch_ref as TR
    saved = TR._swin_attn
    if attn is not None:
        TR._swin_attn = attn
    try:
        return TG.swin(sd, x, labels, dtype=torch.float64, **CFG)
    finally:
        TR._swin_attn = saved


def _record(monkeypatch):
    calls = []
    orig = _lib.call

    def rec(name, *args):
        calls.append((name, args))
        return orig(name, *args)
    monkeypatch.setattr(_lib, "call", rec)
    return calls


def test_rule_launches(monkeypatch):
    import eqxvision_amd as eqv
    sd, x, labels, net, loss_fn, grads_of = _swin()
    names = [k for k in sd if k in _refs(sd, x, labels)[1]]
    calls = _record(monkeypatch)
    loss, g16 = grads_of(names, attn_dtype="bf16")
    seen = [n for n, _ in calls]
    assert seen.count("mv_swin_attn_mp_fwd") == 4 and seen.count("mv_swin_attn_mp_bwd") == 4, seen
    assert "mv_swin_window_attn_bwd_f32" not in seen and "mv_swin_window_attn_fwd" not in seen and "mv_linear_mp_fwd" not in seen
    assert all(a[6] is not None for n, a in calls if n == "mv_swin_attn_mp_bwd"), "trainable tables, yet NULL parts"
    assert np.isfinite(loss)
    ncol = seen.count("mv_colsum_f32")
    del calls[:]
    _, g1 = grads_of(names)
    seen = [n for n, _ in calls]
    assert seen.count("mv_swin_window_attn_fwd") == 4 and seen.count("mv_swin_window_attn_bwd_f32") == 4
    assert not any(n.startswith("mv_swin_attn_mp_f") or n.startswith("mv_swin_attn_mp_bwd") for n in seen)
    assert seen.count("mv_colsum_f32") == ncol, "the two settings do not sum the same number of columns"
    _, g2 = grads_of(names)
    assert all(np.array_equal(g1[n], g2[n]) for n in g1), "the default path is not reproducible"
    # the tables frozen by a filter spec: NULL parts, and four column sums fewer
    tables = {k: v for k, v in sd.items() if k.endswith("relative_position_bias_table")}
    assert len(tables) == 4
    shapes = {tuple(np.shape(v)) for v in tables.values()}
    spec = eqv.tree_map(lambda l: not (np.ndim(l) == 2 and tuple(np.shape(l)) in shapes and np.asarray(l).dtype.kind == "f"), net)
    del calls[:]
    loss3, grads3 = loss_fn(arg=spec, attn_dtype="bf16")(net, x, labels)
    seen = [n for n, _ in calls]
    bw = [a for n, a in calls if n == "mv_swin_attn_mp_bwd"]
    assert len(bw) == 4 and all(a[6] is None for a in bw), "frozen tables, yet the parts were requested"
    assert seen.count("mv_colsum_f32") == ncol - 4 and "mv_scatter_rows_sum_f32" not in seen
    assert np.isfinite(loss3)


def _swin_attn_b(sd, x, p, H, ws, shift):
    """oracle.torch_ref._swin_attn with the core rounding as the contract says (r on q, k, v, dout, P and g; delta, the sums and the
    gradient of the bias un-rounded)."""
    import torch.nn.functional as F

    def r(t):
        return torch.from_numpy(LR.rne_bf16(t.detach().to(torch.float32).numpy()).astype(F64))

    class Core(torch.autograd.Function):
        @staticmethod
        def forward(ctx, q, k, v, extra, scale):
            qr, kr, vr = r(q), r(k), r(v)
            L = qr @ kr.transpose(-2, -1) * scale + extra
            m = L.max(-1, keepdim=True).values
            pe = torch.exp(L - m)
            Z = pe.sum(-1, keepdim=True)
            out = (r(pe) @ vr) / Z
            ctx.save_for_backward(qr, kr, vr, out, L - (m + torch.log(Z)))
            ctx.scale = scale
            return out

        @staticmethod
        def backward(ctx, g):
            qr, kr, vr, out, lp = ctx.saved_tensors
            gr, pr = r(g), torch.exp(lp)
            delta = (g.to(torch.float32).to(torch.float64) * out.to(torch.float32).to(torch.float64)).sum(-1, keepdim=True)
            gl = pr * (gr @ vr.transpose(-2, -1) - delta)
            return ctx.scale * (r(gl) @ kr), ctx.scale * (r(gl).transpose(-2, -1) @ qr), r(pr).transpose(-2, -1) @ gr, gl, None

    B, Hh, Ww, C = x.shape
    shift = [0 if ws[0] >= Hh else shift[0], 0 if ws[1] >= Ww else shift[1]]
    if sum(shift) > 0:
        x = torch.roll(x, (-shift[0], -shift[1]), (1, 2))
    nW, n = (Hh // ws[0]) * (Ww // ws[1]), ws[0] * ws[1]
    x = x.view(B, Hh // ws[0], ws[0], Ww // ws[1], ws[1], C).permute(0, 1, 3, 2, 4, 5).reshape(B * nW, n, C)
    qkv = F.linear(x, sd[p + ".attn.qkv.weight"], sd[p + ".attn.qkv.bias"]).reshape(B * nW, n, 3, H, C // H).permute(2, 0, 3, 1, 4)
    idx = sd[p + ".attn.relative_position_index"].long().view(-1)
    extra = sd[p + ".attn.relative_position_bias_table"][idx].view(n, n, -1).permute(2, 0, 1)[None].expand(B * nW, H, n, n)
    if sum(shift) > 0:
        m = x.new_zeros((Hh, Ww))
        c = 0
        for h in ((0, -ws[0]), (-ws[0], -shift[0]), (-shift[0], None)):
            for w in ((0, -ws[1]), (-ws[1], -shift[1]), (-shift[1], None)):
                m[h[0]:h[1], w[0]:w[1]] = c
                c += 1
        m = m.view(Hh // ws[0], ws[0], Ww // ws[1], ws[1]).permute(0, 2, 1, 3).reshape(nW, n)
        m = m.unsqueeze(1) - m.unsqueeze(2)
        m = m.masked_fill(m != 0, -100.0)
        extra = (extra.reshape(B, nW, H, n, n) + m[None, :, None]).reshape(B * nW, H, n, n)
    y = Core.apply(qkv[0], qkv[1], qkv[2], extra, (C // H) ** -0.5).transpose(1, 2).reshape(B * nW, n, C)
    y = F.linear(y, sd[p + ".attn.proj.weight"], sd[p + ".attn.proj.bias"])
    y = y.view(B, Hh // ws[0], Ww // ws[1], ws[0], ws[1], C).permute(0, 1, 3, 2, 4, 5).reshape(B, Hh, Ww, C)
    return torch.roll(y, (shift[0], shift[1]), (1, 2)) if sum(shift) > 0 else y


def test_swin_model():
    """swin 32 x 32, patch 4, width 32, depths (2, 2), heads (1, 2), window 4, B = 2 (shifted and unshifted blocks; in stage 2 the
    window covers the map), only attn_dtype="bf16".  (a) float64, (b) float64 with the attention core rounding as specified, (c) the
    device's fp32 path; the margins of tests/test_attn_mp_gpu.py::test_vit_model."""
    import eqxvision_amd as eqv
    sd, x, labels, net, loss_fn, grads_of = _swin()
    loss_a, ga = _refs(sd, x, labels)
    loss_b, gb = _refs(sd, x, labels, _swin_attn_b)
    names = [k for k in sd if k in ga]
    flat = lambda g: np.concatenate([np.asarray(g[n], F64).reshape(-1) for n in names])
    loss_bf, g_bf = grads_of(names, attn_dtype="bf16")
    loss_32, g_32 = grads_of(names)
    a, b = flat(ga), flat(gb)
    l2 = lambda u, v: float(np.linalg.norm(u - v) / np.linalg.norm(v))
    d_gpu_b, d_b_a, d_32_a = l2(flat(g_bf), b), l2(b, a), l2(flat(g_32), a)
    print(f"swin/attn_mp: loss bf16 {loss_bf:.6f} fp32 {loss_32:.6f} ref(a) {loss_a:.6f} ref(b) {loss_b:.6f} | rel L2 device-bf16 vs (b) "
          f"{d_gpu_b:.3e}, (b) vs (a) {d_b_a:.3e}, ratio {d_gpu_b / d_b_a:.4f} | device-fp32 vs (a) {d_32_a:.3e}")
    assert np.isfinite(loss_bf)
    for n in names:
        assert np.isfinite(g_bf[n]).all() and np.abs(g_bf[n]).max() > 0, f"{n}: no gradient"
    assert sum(n.endswith("relative_position_bias_table") for n in names) == 4
    assert d_b_a >= 100 * d_32_a, (d_b_a, d_32_a)                    # the rounding is two orders above the fp32 path's own error
    assert d_gpu_b <= 0.25 * d_b_a, (d_gpu_b, d_b_a)

    opt = eqv.optim.adamw(learning_rate=1e-3)
    st = opt.init(eqv.filter(net, eqv.is_array))
    m, fn = net, loss_fn(attn_dtype="bf16")
    for _ in range(2):
        loss, grads = fn(m, x, labels)
        assert np.isfinite(loss)
        updates, st = opt.update(grads, st, eqv.filter(m, eqv.is_array))
        m = eqv.apply_updates(m, updates)
