"""numpy reference of the mixed-precision Swin window attention (csrc/swin_attn_mp.hip: mv_swin_attn_mp_fwd / mv_swin_attn_mp_bwd;
filter_value_and_grad(..., attn_dtype="bf16") on g_swin_window_attention), in the manner of tests/_attn_mp_ref.py: float64 versions of
the contract on r(.) operands, per-element bounds counted from the kernel's roundings, the exact constructions, and a float32
emulation of the kernel with one switch per seeded defect (tests/test_swin_attn_mp_host.py proves the instruments on it;
tests/test_swin_attn_mp_gpu.py applies them to the device).

A shape is (B, Hf, Wf, C, heads, (wh, ww), (sh, sw)).  Everything is per group g = (image, window, head), in that order: q, k, v, dout,
out (G, n, dh), lse (G, n); bias (heads, n, n); the regions of the shift mask (nW, n).  `gather` / `scatter` are the roll and the
window partition between NHWC maps and groups (the statement of tests/_strict.py: swin_bwd64 and tests/_strict_attn.py: swin_pack, for
a rectangular window); `region_map` is swin_bwd64's mask construction.  r(.) = rne_bf16 of tests/_linear_mp_ref.py.

    forward    l = scale r(q) r(k)^T + bias[h] + mask;  pe = exp(l - max l);  Z = sum pe;  out = (pe r(v)) / Z;  lse = max l + log Z
    backward   from q, k, v, dout and the GIVEN out and lse:  p = exp(l - lse);  delta = sum_d dout out;  dp = r(dout) r(v)^T;
               g = p (dp - delta);  dV = p^T r(dout);  dQ = scale g r(k);  dK = scale g^T r(q);  dbias[h] = sum over the groups of head h of g
The references keep p and g un-rounded in float64; that the kernel rounds them to bf16 before the second products is part of the bounds.

Bounds: tests/_attn_mp_ref.py's derivation (u = 2^-24, h(x) = the half ulp of a bf16 value), with
    S_i         = max_j (scale sum_d |q_id k_jd| + |bias_ij| + |mask_ij|): the logit's magnitude now holds the two added terms, and
    dh + 5      roundings of S on a logit instead of dh + 3: the two fp32 additions of bias and mask.  That enters out (numerator and
                denominator: n_ops + 4 S), lse and p (n_p) alike.
    g           e_g = (n_p + 2 dh + 7) u mg, mg = p (|r(dout)| |r(v)|^T + sum_d |dout out|)  (ds of the ViT bound without its scale)
    dQ, dK      scale (E |operand| + n u |g| |operand|) with E = e_g + h(|g| + e_g), then the fp32 product with `scale`: one more
                rounding, u (|ref| + e), then the store's half ulp.
    dV          as in tests/_attn_mp_ref.py.
    parts       part p against the float64 sum of ITS windows (p, p + P, ..): the sum of their e_g plus W u sum |g|, then the store;
                plus W 2^-126: across mask regions p = exp(-100 ..) is a denormal, which the hardware may flush to zero or keep.
    dbias       sum over the head's groups of e_g (g enters un-rounded), plus (W + P + 4) u sum |g|: a part adds its W = ceil(B nW / P)
                windows one after the other in fp32 (W roundings of a partial sum that sum |g| bounds), the P parts are then summed
                in any order (P more), 4 for the column sum's own tree; then the store's half ulp.
"""
import functools

import numpy as np

from tests import _attn_mp_ref as R
from tests import _strict as ST
from tests import _strict_attn as SA
from tests._attn_mp_ref import T, pow2_scale
from tests._linear_mp_ref import rne_bf16

F32, F64 = np.float32, np.float64
U = 2.0 ** -24
LOG2E = F32(1.4426950408889634)
MAX_WGS = 2048                                   # csrc/swin_attn_mp.hip: SWA_MAX_WGS
OUTS = ("out", "lse", "dq", "dk", "dv", "dbias")

# (B, Hf, Wf, C, heads, window, shift): what each covers is in tests/test_swin_attn_mp_gpu.py
SHAPES = ((1, 2, 2, 32, 1, (1, 1), (0, 0)), (2, 4, 6, 32, 1, (2, 3), (1, 1)), (2, 8, 8, 64, 2, (4, 4), (2, 2)),
          (1, 3, 22, 32, 1, (3, 11), (0, 5)), (1, 14, 14, 96, 3, (7, 7), (3, 3)), (1, 14, 14, 96, 3, (7, 7), (0, 0)),
          (1, 16, 8, 128, 2, (8, 8), (4, 0)))
# A workgroup walks MORE than one (image, window) pair: B nW > 2048 / heads and no multiple of P, so the last round is ragged (some
# parts add two windows, the others one).  2080 pairs on 2048 parts with the smallest window; 688 pairs on 682 parts with the
# workload's window, three heads and the shift mask.  At every shape of SHAPES P = B nW and the walk has one step.
WALK_SHAPES = ((130, 8, 8, 32, 1, (2, 2), (1, 1)), (172, 14, 14, 96, 3, (7, 7), (3, 3)))
DEFECTS = ("mask_ignored", "mask_on_unshifted", "pad_key_masked_by_minus100", "bias_transposed", "bias_wrong_head", "roll_wrong_sign",
           "q_prescaled_before_round", "dbias_from_rounded_g", "dbias_drops_last_window", "dbias_part_overwritten")


def shape_id(s):
    B, Hf, Wf, C, heads, (wh, ww), (sh, sw) = s
    return f"{B}x{Hf}x{Wf}x{C}h{heads}w{wh}x{ww}s{sh}x{sw}"


# ------------------------------------------------------------------------------------------------ geometry
def dims(shape):
    """{B, Hf, Wf, C, heads, wh, ww, sh, sw (the shift of an axis whose window covers the map dropped), n, dh, nW, G, shifted}."""
    B, Hf, Wf, C, heads, (wh, ww), (sh, sw) = shape
    sh, sw = (0 if wh >= Hf else sh), (0 if ww >= Wf else sw)
    nW = (Hf // wh) * (Wf // ww)
    return dict(B=B, Hf=Hf, Wf=Wf, C=C, heads=heads, wh=wh, ww=ww, sh=sh, sw=sw, n=wh * ww, dh=C // heads, nW=nW, G=B * nW * heads,
                shifted=sh + sw > 0)


def parts_of(shape):
    """mv_swin_attn_mp_bwd_parts: min(B nW, max(1, 2048 // heads))."""
    d = dims(shape)
    return min(d["B"] * d["nW"], max(1, MAX_WGS // d["heads"]))


def walk_len(shape):
    """W: the (image, window) pairs the busiest workgroup walks, ceil(B nW / P)."""
    d = dims(shape)
    return -(-d["B"] * d["nW"] // parts_of(shape))


def region_map(shape, shift=None):
    """(nW, n) region ids of the rolled map (tests/_strict.py: swin_bwd64); zeros on an unshifted map.  shift: override (a defect)."""
    d = dims(shape)
    sh, sw = (d["sh"], d["sw"]) if shift is None else shift
    m = np.zeros((d["Hf"], d["Wf"]), np.int64)
    if sh + sw > 0:
        c = 0
        for hh in ((0, -d["wh"]), (-d["wh"], -sh), (-sh, None)):
            for wl in ((0, -d["ww"]), (-d["ww"], -sw), (-sw, None)):
                m[hh[0]:hh[1], wl[0]:wl[1]] = c
                c += 1
    return m.reshape(d["Hf"] // d["wh"], d["wh"], d["Wf"] // d["ww"], d["ww"]).transpose(0, 2, 1, 3).reshape(d["nW"], d["n"])


def gather(x, shape, sign=-1):
    """NHWC (B, Hf, Wf, K heads dh) -> (K, G, n, dh): roll by sign * shift (-1: swin.py), partition, split the heads."""
    d = dims(shape)
    K = x.shape[-1] // d["C"]
    if d["shifted"]:
        x = np.roll(x, (sign * d["sh"], sign * d["sw"]), (1, 2))
    t = x.reshape(d["B"], d["Hf"] // d["wh"], d["wh"], d["Wf"] // d["ww"], d["ww"], K, d["heads"], d["dh"])
    return np.ascontiguousarray(t.transpose(5, 0, 1, 3, 6, 2, 4, 7).reshape(K, d["G"], d["n"], d["dh"]))


def scatter(t, shape, sign=-1):
    """The inverse of gather: (K, G, n, dh) -> NHWC."""
    d = dims(shape)
    K = t.shape[0]
    x = t.reshape(K, d["B"], d["Hf"] // d["wh"], d["Wf"] // d["ww"], d["heads"], d["wh"], d["ww"], d["dh"])
    x = x.transpose(1, 2, 5, 3, 6, 0, 4, 7).reshape(d["B"], d["Hf"], d["Wf"], K * d["C"])
    if d["shifted"]:
        x = np.roll(x, (-sign * d["sh"], -sign * d["sw"]), (1, 2))
    return np.ascontiguousarray(x)


def group_regions(shape, reg=None):
    """(G, n): the regions of every group."""
    d = dims(shape)
    reg = region_map(shape) if reg is None else reg
    return np.broadcast_to(reg[None, :, None], (d["B"], d["nW"], d["heads"], d["n"])).reshape(d["G"], d["n"])


def extra_of(shape, bias, reg=None, masked=True):
    """(G, n, n) float64: bias[head] + (-100 where the regions differ, on a shifted map)."""
    d = dims(shape)
    gr = group_regions(shape, reg)
    am = np.where(gr[:, :, None] != gr[:, None, :], -100.0, 0.0) if masked else 0.0
    hb = np.broadcast_to(np.asarray(bias, F64)[None, None], (d["B"], d["nW"], d["heads"], d["n"], d["n"])).reshape(d["G"], d["n"], d["n"])
    return hb + am


def part_sum(g, shape):
    """(G, n, n) -> (P, heads, n, n): part p holds the pairs p, p + P, p + 2 P, .. (csrc/swin_attn_mp.hip)."""
    d = dims(shape)
    Pn, W, pairs = parts_of(shape), walk_len(shape), d["B"] * d["nW"]
    t = np.zeros((W * Pn, d["heads"], d["n"], d["n"]), g.dtype)
    t[:pairs] = g.reshape(pairs, d["heads"], d["n"], d["n"])
    return t.reshape(W, Pn, d["heads"], d["n"], d["n"]).sum(0)


def head_sum(g, shape):
    """(G, n, n) -> (heads, n, n): summed over images and windows."""
    d = dims(shape)
    return g.reshape(d["B"] * d["nW"], d["heads"], d["n"], d["n"]).sum(0)


# ------------------------------------------------------------------------------------------------ float64 references
def fwd64(c, rnd=rne_bf16):
    q, k, v = (np.asarray(rnd(c[t]), F64) for t in ("q", "k", "v"))
    ex = extra_of(c["shape"], c["bias"])
    L = q @ T(k) * c["scale"] + ex
    m = L.max(-1, keepdims=True)
    pe = np.exp(L - m)
    Z = pe.sum(-1, keepdims=True)
    pr = pe / Z
    return {"out": pr @ v, "lse": (m + np.log(Z))[..., 0], "probs": pr, "mag": pr @ np.abs(v),
            "smag": (np.abs(q) @ T(np.abs(k)) * c["scale"] + np.abs(ex)).max(-1, keepdims=True),
            "e_p": (ST.half_ulp_out(pe, "bf16") @ np.abs(v)) / Z, "logz": np.log(Z)[..., 0]}


def bwd64(c, out, lse, rnd=rne_bf16):
    """{"dq", "dk", "dv", "dbias", "p", "g", "mg"} in float64 from the given out and lse."""
    q, k, v, go = (np.asarray(rnd(c[t]), F64) for t in ("q", "k", "v", "dout"))
    sc = c["scale"]
    p = np.exp(q @ T(k) * sc + extra_of(c["shape"], c["bias"]) - np.asarray(lse, F64)[..., None])
    do = np.asarray(c["dout"], F64) * np.asarray(out, F64)
    g = p * (go @ T(v) - do.sum(-1, keepdims=True))
    mg = p * (np.abs(go) @ T(np.abs(v)) + np.abs(do).sum(-1, keepdims=True))
    return {"dq": sc * (g @ k), "dk": sc * (T(g) @ q), "dv": T(p) @ go, "dbias": head_sum(g, c["shape"]), "p": p, "g": g, "mg": mg}


# ------------------------------------------------------------------------------------------------ bounds (module docstring)
_store = R._store


def fwd_bounds(f, n, dh):
    nops = SA.n_ops(f["smag"], n, dh) + 4 * f["smag"]
    e_out = f["e_p"] + nops * U * f["mag"]
    e_lse = ((dh + 5) * f["smag"][..., 0] + n + 8 + 2 * np.abs(f["logz"])) * U
    return {"out": _store(f["out"], e_out), "lse": _store(f["lse"], e_lse)}


def bwd_bounds(b, c, smag, rnd=rne_bf16):
    q, k, go = (np.abs(np.asarray(rnd(c[t]), F64)) for t in ("q", "k", "dout"))
    n, dh = q.shape[1:]
    sc, shape = c["scale"], c["shape"]
    n_p = (dh + 5) * smag + 3 * (2 * smag + 6) + 2
    e_g = (n_p + 2 * dh + 7) * U * b["mg"]
    ag = np.abs(b["g"])
    E = e_g + ST.half_ulp_out(ag + e_g, "bf16")
    Ep = n_p * U * b["p"] + ST.half_ulp_out(b["p"] * (1 + n_p * U), "bf16")

    def scaled(ref, e):
        e = sc * e
        return _store(ref, e + U * (np.abs(ref) + e))
    d = dims(shape)
    Pn = parts_of(shape)
    W = -(-d["B"] * d["nW"] // Pn)
    e_db = head_sum(e_g, shape) + (W + Pn + 4) * U * head_sum(ag, shape)
    b["parts"] = part_sum(b["g"], shape)                                  # each part on its own: W roundings, no column sum
    e_parts = _store(b["parts"], part_sum(e_g, shape) + W * U * part_sum(ag, shape) + W * 2.0 ** -126)
    return {"parts": e_parts, "dq": scaled(b["dq"], E @ k + n * U * (ag @ k)), "dk": scaled(b["dk"], T(E) @ q + n * U * (T(ag) @ q)),
            "dv": _store(b["dv"], T(Ep) @ go + n * U * (T(b["p"]) @ go)), "dbias": _store(b["dbias"], e_db)}


# ------------------------------------------------------------------------------------------------ cases
def gauss_shape(shape):
    """The shape with B raised until the output has 8192 elements: the rounding bias needs its 4096 at the small shapes too."""
    B, Hf, Wf, C = shape[:4]
    return (max(B, -(-8192 // (Hf * Wf * C))),) + tuple(shape[1:])


@functools.lru_cache(maxsize=None)
def gauss_case(shape, seed=41):
    """fp32 Gaussian q, k, v, dout (NOT bf16 values), bias 0.5 N(0, 1), scale dh^-0.5, at gauss_shape(shape)."""
    shape = gauss_shape(shape)
    d = dims(shape)
    rng = ST.rng_of(seed)
    q, k, v, dout = (rng.standard_normal((d["G"], d["n"], d["dh"])).astype(F32) for _ in range(4))
    bias = (0.5 * rng.standard_normal((d["heads"], d["n"], d["n"]))).astype(F32)
    return {"kind": "gauss", "shape": shape, "q": q, "k": k, "v": v, "dout": dout, "bias": bias, "scale": float(d["dh"] ** -0.5)}


@functools.lru_cache(maxsize=None)
def exact_case(kind, shape, seed=47):
    """select / tie / flat of tests/_strict_attn.py by key codes, the winners inside the query's mask region, with a power-of-two scale,
    the v / dout of tests/_attn_mp_ref.py: exact_case for the backward, and an integer-valued bias that is constant along the keys:
    bias[h][i][:] = c(h, i) in [-3, 3].  It moves every logit of a row alike -- the winners, the gaps and the probabilities stay what the
    construction says and lse moves by c(h, i) exactly -- but read transposed it differs between the two winners of a tie (and breaks
    it), and read from another head it moves lse."""
    d = dims(shape)
    G, n, dh = d["G"], d["n"], d["dh"]
    scale = pow2_scale(dh)
    p = dict(SA.build(kind, G, n, dh, scale, seed, regions=group_regions(shape)))
    rng = ST.rng_of(seed + 1)
    if kind == "select":
        p["v"] = ST.int_tensor(rng, (G, n, dh), 8)
        p["dout"] = ST.int_tensor(rng, (G, n, dh), 4)
    elif kind == "tie":
        sign = rng.choice([-1.0, 1.0], (G, 1, dh))
        p["v"] = (sign * rng.integers(192, 256, (G, n, dh))).astype(F32)
        dout = np.zeros((G, n, dh), F32)
        cc = rng.choice([-4.0, -2.0, -1.0, 1.0, 2.0, 4.0], (G, n))
        np.put_along_axis(dout, rng.integers(0, dh, (G, n))[..., None], cc[..., None].astype(F32), -1)
        p["dout"] = dout
    else:
        p["dout"] = ST.int_tensor(rng, (G, n, dh), 4)
    p["bias"] = np.broadcast_to(ST.int_tensor(rng, (d["heads"], n, 1), 3), (d["heads"], n, n)).copy()
    p["shape"] = shape
    cnt = p["win"].sum(-1, keepdims=True).astype(F64)
    p["P"] = p["win"] / cnt
    p["expect"] = p["P"] @ p["v"].astype(F64)
    L = SA.logits64(p, extra_of(shape, p["bias"]))
    p["lse_expect"] = np.where(p["win"], L, -np.inf).max(-1) + np.log(cnt[..., 0])
    for t in ("q", "k", "v", "dout", "bias"):
        assert np.array_equal(rne_bf16(p[t]), p[t]), f"{kind}: {t} must be bf16 values"
    return p


@functools.lru_cache(maxsize=None)
def has_tie(shape):
    """A tie needs, for at least half of the rows, two keys of one mask region whose codes differ in one bit (SA.build asserts it):
    not with a single key, nor where the shift cuts a small window into regions of one or two tokens."""
    if dims(shape)["n"] < 2:
        return False
    try:
        exact_case("tie", shape)
    except AssertionError:
        return False
    return True


def exact_bwd_ref(p):
    """float64 gradients of an exact case from the EXACT probabilities win / count."""
    q, k, v, go = (p[t].astype(F64) for t in ("q", "k", "v", "dout"))
    dp = go @ T(v)
    g = p["P"] * (dp - (p["P"] * dp).sum(-1, keepdims=True))
    return {"dq": p["scale"] * (g @ k), "dk": p["scale"] * (T(g) @ q), "dv": T(p["P"]) @ go, "g": g, "dbias": head_sum(g, p["shape"])}


def tie_eps(p):
    """The relative error of the kernel's p = exp(l - lse) on a tie, the one inexact factor of the un-rounded g (tests/_attn_mp_ref.py)."""
    return float((ST.half_ulp_out(np.abs(p["lse_expect"]), "fp32") + 8 * U).max())


def prove_exact_case(p):
    """The CPU proof of a construction, before any output is looked at."""
    SA.prove(p, extra_of(p["shape"], p["bias"]))
    if p["kind"] == "flat":
        return
    r = exact_bwd_ref(p)
    q, k, go, g = np.abs(p["q"].astype(F64)), np.abs(p["k"].astype(F64)), np.abs(p["dout"].astype(F64)), r["g"]
    assert np.array_equal(rne_bf16(g.astype(F32)).astype(F64), g), "g is not a bf16 value"
    for t, a, b in (("dq", np.abs(g), k), ("dk", T(np.abs(g)), q), ("dv", T(p["P"]), go)):
        assert (a @ b * 4).max() < ST.ACC_INT_MAX and np.array_equal(r[t].astype(F32).astype(F64), r[t]), f"{t}: not exact in fp32"
    assert np.abs(p["dout"].astype(F64) * p["expect"]).sum(-1).max() * 2 < ST.ACC_INT_MAX              # delta: multiples of 1/2
    if p["kind"] == "select":
        assert not r["dq"].any() and not r["dk"].any() and not r["dbias"].any()
        assert np.array_equal(r["dv"], T(p["win"].astype(F64)) @ p["dout"].astype(F64))
    else:
        assert np.abs(r["dq"]).max() > 0 and np.abs(r["dk"]).max() > 0 and np.abs(r["dbias"]).max() > 0
        assert tie_eps(p) < 2.0 ** -12, "tie: p would not round to 0.5"


# ------------------------------------------------------------------------------------------------ checks
_info = R._info
worst = R.worst


def check_exact_fwd(got, p):
    n = p["win"].shape[-1]
    parts = {"out": SA.check_exactish(p["kind"], got["out"], p, out="fp32", n=n)}
    if p["kind"] != "flat":
        parts["lse"] = ST.check_bound(got["lse"], p["lse_expect"], None, 0, "fp32", bound=2.0 ** -21 * np.abs(p["lse_expect"]))
    return _info(**parts)


def check_exact_bwd(got, p):
    """dQ, dK, dV bit-equal to float64.  dbias: exactly 0 on select (every g is 0); on tie the un-rounded g carries p's relative error
    tie_eps, and the sums their W + P + 4 roundings (module docstring)."""
    r = exact_bwd_ref(p)
    parts = {t: ST.check_exact(got[t], r[t]) for t in ("dq", "dk", "dv")}
    if p["kind"] == "select":
        parts["dbias"] = ST.check_exact(got["dbias"], r["dbias"])
    else:
        d = dims(p["shape"])
        Pn = parts_of(p["shape"])
        W = -(-d["B"] * d["nW"] // Pn)
        parts["dbias"] = ST.check_bound(got["dbias"], r["dbias"], None, 0, "fp32",
                                        bound=(tie_eps(p) + (W + Pn + 4) * U) * head_sum(np.abs(r["g"]), p["shape"]))
    return _info(**parts)


def check_gauss(got, c):
    """Per element against float64 on the rounded operands, all six outputs; the rounding bias of `out` and `dv`.  The backward's
    references start from got["out"], got["lse"]."""
    n, dh = c["q"].shape[1:]
    f = fwd64(c)
    fb = fwd_bounds(f, n, dh)
    parts = {t: ST.check_bound(got[t], f[t], None, 0, "fp32", bound=fb[t]) for t in ("out", "lse")}
    if np.isfinite(np.asarray(got["lse"], F64)).all() and np.isfinite(np.asarray(got["out"], F64)).all():
        b = bwd64(c, got["out"], got["lse"])
        bb = bwd_bounds(b, c, f["smag"])
        for t in ("dq", "dk", "dv", "dbias", "parts"):
            parts[t] = ST.check_bound(got[t], b[t], None, 0, "fp32", bound=bb[t])
        for t, ref in (("out", f["out"]), ("dv", b["dv"])):
            bias, nb = ST.rounding_bias(got[t], ref, "bf16")
            parts[t + "_bias"] = {"ok": bool(nb >= ST.BIAS_MIN_ELEMS and abs(bias) <= ST.BIAS_LIMIT), "bias": bias, "n_bias": nb}
    else:
        parts["dq"] = {"ok": False, "err": "forward not finite"}
    return _info(**parts)


# ------------------------------------------------------------------------------------------------ emulator
def emulate(c, **defect):
    """float32 model of swin_attn_mp.hip on a case: {"out", "lse", "dq", "dk", "dv", "dbias", "parts"}.  One defect per switch:
      mask_ignored                no -100 between regions
      mask_on_unshifted           an unshifted map is masked as if it were shifted by half a window
      pad_key_masked_by_minus100  a padded key gets the logit 0 - 100 instead of -inf (forward)
      bias_transposed             bias[h][j][i]
      bias_wrong_head             bias[(h + 1) % heads]
      roll_wrong_sign             rows gathered and scattered with the roll reversed (the mask stays where it is)
      q_prescaled_before_round    r(q scale) instead of scale (r(q) . r(k))
      dbias_from_rounded_g        the bias gradient sums r(g)
      dbias_drops_last_window     the last (image, window) pair is not added
      dbias_part_overwritten      a part holds the g of the last window it walked, not their sum (shows only where W > 1)"""
    assert not set(defect) - set(DEFECTS), defect
    shape = c["shape"]
    d = dims(shape)
    G, n, dh, heads = d["G"], d["n"], d["dh"], d["heads"]
    q, k, v, do = (np.asarray(c[t], F32) for t in ("q", "k", "v", "dout"))
    if defect.get("roll_wrong_sign"):
        q, k, v = gather(scatter(np.stack([q, k, v]), shape), shape, sign=+1)
        do = gather(scatter(do[None], shape), shape, sign=+1)[0]
    sc = F32(c["scale"])
    pre = bool(defect.get("q_prescaled_before_round"))
    qr, kr, vr, gr = rne_bf16(q * sc if pre else q), rne_bf16(k), rne_bf16(v), rne_bf16(do)
    NP = 64
    kp, vp = np.zeros((G, NP, dh), F32), np.zeros((G, NP, dh), F32)
    kp[:, :n], vp[:, :n] = kr, vr
    bias = np.asarray(c["bias"], F32)
    if defect.get("bias_transposed"):
        bias = np.ascontiguousarray(T(bias))
    if defect.get("bias_wrong_head"):
        bias = np.roll(bias, -1, 0)
    reg = region_map(shape)
    if defect.get("mask_on_unshifted") and not d["shifted"]:
        reg = region_map(shape, (0 if d["wh"] >= d["Hf"] else d["wh"] // 2, 0 if d["ww"] >= d["Wf"] else d["ww"] // 2))
    ex = np.zeros((G, n, NP), F32)
    ex[:, :, :n] = extra_of(shape, bias, reg, masked=not defect.get("mask_ignored")).astype(F32)
    s = qr @ T(kp)
    L = ((s if pre else s * sc) + ex).astype(F32)
    Lf = L.copy()
    Lf[:, :, n:] = F32(-100.0) if defect.get("pad_key_masked_by_minus100") else F32(-np.inf)
    mx = Lf.max(-1, keepdims=True)
    with np.errstate(under="ignore"):
        pe = np.exp2((Lf - mx) * LOG2E).astype(F32)
    Z = pe.sum(-1, keepdims=True, dtype=F32)
    out = ((rne_bf16(pe) @ vp) * (F32(1) / Z)).astype(F32)
    lse = (mx + np.log(Z)).astype(F32)[..., 0]
    with np.errstate(all="ignore"):
        p = np.exp2(((L - lse[..., None]) * LOG2E).astype(F32)).astype(F32)
        p[:, :, n:] = 0
        delta = (do * out).sum(-1, keepdims=True, dtype=F32)
        g = (p * (gr @ T(vp) - delta)).astype(F32)
        gb, pb = rne_bf16(g), rne_bf16(p)
        one = F32(1) if pre else sc
        dq = ((gb @ kp) * sc).astype(F32)
        dk = ((T(gb) @ qr) * one).astype(F32)[:, :n]
        dv = (T(pb) @ gr).astype(F32)[:, :n]
    Pn = parts_of(shape)
    pairs = d["B"] * d["nW"]
    src = (gb if defect.get("dbias_from_rounded_g") else g)[:, :, :n].reshape(pairs, heads, n, n)
    parts = np.zeros((Pn, heads, n, n), F32)
    last = pairs - 1 if defect.get("dbias_drops_last_window") else pairs
    for pt in range(Pn):
        for t in range(pt, last, Pn):
            parts[pt] = src[t] if defect.get("dbias_part_overwritten") else parts[pt] + src[t]
    res = {"out": out, "lse": lse, "dq": dq, "dk": dk, "dv": dv}
    if defect.get("roll_wrong_sign"):
        res["out"] = gather(scatter(out[None], shape, sign=+1), shape)[0]
        res["dq"], res["dk"], res["dv"] = gather(scatter(np.stack([dq, dk, dv]), shape, sign=+1), shape)
    res["parts"] = parts
    res["dbias"] = parts.sum(0, dtype=F32)
    return res
