"""numpy reference of the mixed-precision attention core (csrc/attn_mp.hip: mv_mha_mp_fwd / mv_mha_mp_bwd;
filter_value_and_grad(..., attn_dtype="bf16")): float64 versions of the contract on r(.) operands, per-element bounds counted from the
kernel's roundings, the exact constructions, and a float32 emulation of the kernel with one switch per seeded defect
(tests/test_attn_mp_host.py proves the instruments on it; tests/test_attn_mp_gpu.py applies them to the device).

Everything is per group g = (image, head): q, k, v, dout, out (G, n, dh), lse (G, n).  r(.) = rne_bf16 of tests/_linear_mp_ref.py.

    forward    s = r(q) r(k)^T;  l = scale s;  pe = exp(l - max l);  Z = sum pe;  out = (pe r(v)) / Z;  lse = max l + log Z
    backward   from q, k, v, dout and the GIVEN out and lse (what the forward stored: the reference does not re-derive them, so that a
               forward error is not counted twice):  p = exp(l - lse);  delta = sum_d dout out;  dp = r(dout) r(v)^T;
               ds = scale p (dp - delta);  dV = p^T r(dout);  dQ = ds r(k);  dK = ds^T r(q)
The references keep p and ds un-rounded in float64; that the kernel rounds them to bf16 before the second products is part of the
bounds (as the rounding of P is in tests/_strict_attn.py's Gaussian bound).

Bounds (u = 2^-24, h(x) = the half ulp of a bf16 value, S_i = max_j sum_d |q_id k_jd| scale, N keys, |x| element-wise):
    out, probs  SA.mfma_bound / SA.n_ops with an fp32 store: a logit carries dh + 3 roundings of S (the maximum's own error
                shifts numerator and denominator alike and cancels), the sums N each, exp / rcp / products 8.
    lse         e = ((dh + 3) S + N + 8 + 2 |log Z|) u: the logit error passes into a soft maximum with weights that sum to 1, a
                relative error of Z is an absolute error of its logarithm, the logarithm's own rounding; then the final sum's
                half ulp of |lse| + e.
    p           relative eps_p = ((dh + 3) S + 3 (2 S + 6) + 2) u: the logit, then the difference to lse, the product with
                log2(e) and its constant (three roundings of |l - lse| <= 2 S + log 256), v_exp_f32 (2).
    ds          e_ds = (n_p + 2 dh + 7) u mds with mds = scale p (|r(dout)| |r(v)|^T + sum_d |dout out|): p's error, dh
                accumulations of dp, dh + 2 of delta, the difference and the two products.
    dQ, dK      E = e_ds + h(|ds| + e_ds) per element of ds (the bf16 rounding), carried through the product with |r(k)| / |r(q)|,
                plus N u (|ds| . |operand|) for the fp32 accumulation, plus the store's half ulp.
    dV          the same with E_p = eps_p p + h(p (1 + eps_p)) and |r(dout)|.
"""
import functools

import numpy as np

from tests import _strict as ST
from tests import _strict_attn as SA
from tests._linear_mp_ref import rne_bf16, trunc_bf16
from tests._strict_attn import build as _sa_build  # select / tie / flat: the key-code constructions
from tests._strict_attn import gain, mha_groups, mha_pack  # noqa: F401  (re-exported to the tests)

F32, F64 = np.float32, np.float64
U = 2.0 ** -24
LOG2E = F32(1.4426950408889634)
OUTS = ("out", "lse", "dq", "dk", "dv")

# (B, H, N, dh): a single key, a ragged first tile, one key past a tile in each MFMA width, the workload's N, the limit
SHAPES = ((1, 1, 1, 32), (1, 1, 5, 32), (2, 3, 17, 32), (1, 2, 33, 64), (1, 1, 64, 64), (2, 2, 65, 64), (1, 1, 197, 64), (1, 1, 256, 64))
DEFECTS = ("drop_last_key", "unmasked_pad", "truncate_p", "delta_rounded", "no_scale_ds", "swap_dk_dv", "skip_last_query_tile",
           "lse_no_max")


def shape_id(s):
    return "x".join(str(v) for v in s)


def pow2_scale(dh):
    """The power of two at or below dh^-0.5 (dh = 64: dh^-0.5 itself)."""
    return float(2.0 ** np.floor(np.log2(dh ** -0.5)))


def T(a):
    return np.swapaxes(a, -1, -2)


# ------------------------------------------------------------------------------------------------ float64 references
def fwd64(q, k, v, scale, rnd=rne_bf16):
    """{"out", "lse", "probs", "mag" (sum_j p_j |v_j|), "smag" (S, (G, n, 1)), "e_p" (the worst case of rounding pe to bf16), "logz"}."""
    q, k, v = (np.asarray(rnd(t), F64) for t in (q, k, v))
    L = q @ T(k) * scale
    m = L.max(-1, keepdims=True)
    pe = np.exp(L - m)
    Z = pe.sum(-1, keepdims=True)
    pr = pe / Z
    return {"out": pr @ v, "lse": (m + np.log(Z))[..., 0], "probs": pr, "mag": pr @ np.abs(v),
            "smag": (np.abs(q) @ T(np.abs(k)) * scale).max(-1, keepdims=True), "e_p": (ST.half_ulp_out(pe, "bf16") @ np.abs(v)) / Z,
            "logz": np.log(Z)[..., 0]}


def bwd64(q, k, v, out, dout, lse, scale, rnd=rne_bf16):
    """The lse form: {"dq", "dk", "dv", "p", "ds", "mds"} in float64 from the given out and lse."""
    q, k, v, g = (np.asarray(rnd(t), F64) for t in (q, k, v, dout))
    p = np.exp(q @ T(k) * scale - np.asarray(lse, F64)[..., None])
    delta = (np.asarray(dout, F64) * np.asarray(out, F64)).sum(-1, keepdims=True)
    dp = g @ T(v)
    ds = scale * p * (dp - delta)
    mds = scale * p * (np.abs(g) @ T(np.abs(v)) + np.abs(np.asarray(dout, F64) * np.asarray(out, F64)).sum(-1, keepdims=True))
    return {"dq": ds @ k, "dk": T(ds) @ q, "dv": T(p) @ g, "p": p, "ds": ds, "mds": mds}


def bwd64_probs(q, k, v, probs, dout, scale, rnd=rne_bf16):
    """The kept-probabilities form of train_bwd.hip: dS = scale P (dP - sum_j P dP)."""
    q, k, v, g = (np.asarray(rnd(t), F64) for t in (q, k, v, dout))
    P = np.asarray(probs, F64)
    dp = g @ T(v)
    ds = scale * P * (dp - (P * dp).sum(-1, keepdims=True))
    return {"dq": ds @ k, "dk": T(ds) @ q, "dv": T(P) @ g}


# ------------------------------------------------------------------------------------------------ bounds (module docstring)
def _store(ref, e):
    return e + ST.half_ulp_out(np.abs(ref) + e, "fp32")


def fwd_bounds(f, n, dh):
    nops = SA.n_ops(f["smag"], n, dh)
    e_out = f["e_p"] + nops * U * f["mag"]
    e_lse = ((dh + 3) * f["smag"][..., 0] + n + 8 + 2 * np.abs(f["logz"])) * U
    return {"out": _store(f["out"], e_out), "lse": _store(f["lse"], e_lse), "probs": nops * U * f["probs"]}


def bwd_bounds(b, q, k, dout, smag, n, dh, rnd=rne_bf16):
    q, k, g = (np.abs(np.asarray(rnd(t), F64)) for t in (q, k, dout))
    n_p = (dh + 3) * smag + 3 * (2 * smag + 6) + 2                       # (G, n, 1)
    e_ds = (n_p + 2 * dh + 7) * U * b["mds"]
    E = e_ds + ST.half_ulp_out(np.abs(b["ds"]) + e_ds, "bf16")
    ads = np.abs(b["ds"])
    Ep = n_p * U * b["p"] + ST.half_ulp_out(b["p"] * (1 + n_p * U), "bf16")
    return {"dq": _store(b["dq"], E @ k + n * U * (ads @ k)), "dk": _store(b["dk"], T(E) @ q + n * U * (T(ads) @ q)),
            "dv": _store(b["dv"], T(Ep) @ g + n * U * (T(b["p"]) @ g))}


# ------------------------------------------------------------------------------------------------ cases
def gauss_shape(shape):
    """(B, H, N, dh) with B raised until B H N dh >= 8192: the rounding bias needs its 4096 elements at the small shapes too."""
    B, H, N, dh = shape
    return (max(B, -(-8192 // (H * N * dh))), H, N, dh)


@functools.lru_cache(maxsize=None)
def gauss_case(shape, seed=31):
    """fp32 Gaussian operands (NOT bf16 values: the rounding r(.) is part of what is tested)."""
    B, H, N, dh = gauss_shape(shape)
    rng = ST.rng_of(seed)
    q, k, v, dout = (rng.standard_normal((B * H, N, dh)).astype(F32) for _ in range(4))
    return {"kind": "gauss", "q": q, "k": k, "v": v, "dout": dout, "scale": float(dh ** -0.5), "B": B, "H": H}


@functools.lru_cache(maxsize=None)
def exact_case(kind, shape, seed=37):
    """select / tie / flat of tests/_strict_attn.py with a power-of-two scale and operands of this module's own for the backward:
    select  v integers in [-8, 8], dout integers in [-4, 4]: P is one-hot, delta equals dp at the winner, so dQ = dK = 0 and
            dV_j = sum of the dout_i with pi(i) = j, all exact.
    tie     v = sign_d * m with m an integer in [192, 255] (one sign per channel), dout_i = c_i e_{d_i} with c_i a signed power of
            two <= 4: out = (v_a + v_b) / 2 is exact in fp32 but NO bf16 value where the sum is odd (a delta from rounded operands is
            off by c / 2); dp_a - delta = c (v_a - v_b) / 2 with |v_a - v_b| <= 63, so the exact ds = scale c (v_a - v_b) / 4 is a bf16
            value.  The kernel's p = exp(l - lse) is 0.5 (1 + eps), |eps| <= half_ulp(|lse|) + 8 u << 2^-9 -- the one inexact factor --
            so r(p) = 0.5 and r(ds) = the exact ds: dQ, dK and dV are bit-equal to the float64 values (`prove_tie_bwd`).
    flat    forward only: every real logit <= -128, a padded key at 0 would win."""
    B, H, N, dh = shape
    G = B * H
    scale = pow2_scale(dh)
    p = dict(_sa_build(kind, G, N, dh, scale, seed))
    rng = ST.rng_of(seed + 1)
    if kind == "select":
        p["v"] = ST.int_tensor(rng, (G, N, dh), 8)
        p["dout"] = ST.int_tensor(rng, (G, N, dh), 4)
    elif kind == "tie":
        sign = rng.choice([-1.0, 1.0], (G, 1, dh))
        p["v"] = (sign * rng.integers(192, 256, (G, N, dh))).astype(F32)
        dout = np.zeros((G, N, dh), F32)
        c = rng.choice([-4.0, -2.0, -1.0, 1.0, 2.0, 4.0], (G, N))
        d = rng.integers(0, dh, (G, N))
        np.put_along_axis(dout, d[..., None], c[..., None].astype(F32), -1)
        p["dout"] = dout
    else:
        p["dout"] = ST.int_tensor(rng, (G, N, dh), 4)
    cnt = p["win"].sum(-1, keepdims=True).astype(F64)
    p["P"] = p["win"] / cnt
    p["expect"] = p["P"] @ p["v"].astype(F64)
    L = SA.logits64(p)
    p["lse_expect"] = np.where(p["win"], L, -np.inf).max(-1) + np.log(cnt[..., 0])
    p["B"], p["H"] = B, H
    for t in ("q", "k", "v", "dout"):
        assert np.array_equal(rne_bf16(p[t]), p[t]), f"{kind}: {t} must be bf16 values"
    return p


def has_tie(shape):
    """A tie needs two keys."""
    return shape[2] >= 2


def exact_bwd_ref(p):
    """float64 gradients of an exact case from the EXACT probabilities win / count."""
    return bwd64_probs(p["q"], p["k"], p["v"], p["P"], p["dout"], p["scale"])


def prove_exact_case(p):
    """The CPU proof of a construction, before any output is looked at."""
    SA.prove(p)
    if p["kind"] == "flat":
        return
    r = exact_bwd_ref(p)
    q, k, v, g = (p[t].astype(F64) for t in ("q", "k", "v", "dout"))
    dp = g @ T(v)
    ds = p["scale"] * p["P"] * (dp - (p["P"] * dp).sum(-1, keepdims=True))
    assert np.array_equal(rne_bf16(ds.astype(F32)).astype(F64), ds), "ds is not a bf16 value"
    for t, a, b in (("dq", np.abs(ds), np.abs(k)), ("dk", T(np.abs(ds)), np.abs(q)), ("dv", T(p["P"]), np.abs(g))):
        assert (a @ b / (p["scale"] / 4)).max() < ST.ACC_INT_MAX and np.array_equal(r[t].astype(F32).astype(F64), r[t]), f"{t}: not exact in fp32"
    assert np.abs(p["dout"].astype(F64) * p["expect"]).sum(-1).max() * 2 < ST.ACC_INT_MAX              # delta: multiples of 1/2
    if p["kind"] == "select":
        assert not r["dq"].any() and not r["dk"].any() and np.array_equal(r["dv"], T(p["win"].astype(F64)) @ g)
    else:
        two = p["win"].sum(-1) == 2
        odd = (np.rint(2 * p["expect"]) % 2 == 1) & two[..., None] & (p["dout"] != 0)
        assert odd.sum() >= 1, "tie: no delta term with an out that is not a bf16 value"
        assert np.abs(r["dq"]).max() > 0 and np.abs(r["dk"]).max() > 0
        eps = ST.half_ulp_out(np.abs(p["lse_expect"]), "fp32") + 8 * U
        assert eps.max() < 2.0 ** -12, "tie: p would not round to 0.5"


# ------------------------------------------------------------------------------------------------ checks
def _info(**parts):
    parts["ok"] = all(v["ok"] for v in parts.values())
    return parts


def check_exact_fwd(got, p):
    """out and lse of select / tie (within 2^-21 relative: SA.check_exactish's fp32 store) or flat ((N + 8) 2^-24)."""
    n = p["win"].shape[-1]
    parts = {"out": SA.check_exactish(p["kind"], got["out"], p, out="fp32", n=n)}
    if p["kind"] != "flat":
        parts["lse"] = ST.check_bound(got["lse"], p["lse_expect"], None, 0, "fp32", bound=2.0 ** -21 * np.abs(p["lse_expect"]))
    return _info(**parts)


def check_exact_bwd(got, p):
    r = exact_bwd_ref(p)
    return _info(**{t: ST.check_exact(got[t], r[t]) for t in ("dq", "dk", "dv")})


def check_gauss(got, c, probs=None):
    """Per element against float64 on the rounded operands, all five outputs; the rounding bias of `out` and `dv` (where the bf16
    rounding of P lands).  `got`: the kernel's out, lse, dq, dk, dv -- the backward's references start from got["out"], got["lse"]."""
    n, dh = c["q"].shape[1:]
    f = fwd64(c["q"], c["k"], c["v"], c["scale"])
    fb = fwd_bounds(f, n, dh)
    parts = {t: ST.check_bound(got[t], f[t], None, 0, "fp32", bound=fb[t]) for t in ("out", "lse")}
    if probs is not None:
        parts["probs"] = ST.check_bound(probs, f["probs"], None, 0, "fp32", bound=fb["probs"])
    if np.isfinite(np.asarray(got["lse"], F64)).all() and np.isfinite(np.asarray(got["out"], F64)).all():
        b = bwd64(c["q"], c["k"], c["v"], got["out"], c["dout"], got["lse"], c["scale"])
        bb = bwd_bounds(b, c["q"], c["k"], c["dout"], f["smag"], n, dh)
        for t in ("dq", "dk", "dv"):
            parts[t] = ST.check_bound(got[t], b[t], None, 0, "fp32", bound=bb[t])
        for t, ref in (("out", f["out"]), ("dv", b["dv"])):
            bias, nb = ST.rounding_bias(got[t], ref, "bf16")
            parts[t + "_bias"] = {"ok": bool(nb >= ST.BIAS_MIN_ELEMS and abs(bias) <= ST.BIAS_LIMIT), "bias": bias, "n_bias": nb}
    else:
        parts["dq"] = {"ok": False, "err": "forward not finite"}
    return _info(**parts)


def worst(info):
    """{entry: worst |got - ref| / bound} of a check_gauss verdict."""
    return {t: v.get("worst", float("nan")) for t, v in info.items() if isinstance(v, dict) and "worst" in v}


# ------------------------------------------------------------------------------------------------ emulator
def emulate(c, want_probs=False, **defect):
    """float32 model of attn_mp.hip on a case's q, k, v, dout: {"out", "lse", "dq", "dk", "dv"[, "probs"]}.  One defect per switch:
      drop_last_key         key n - 1 is masked like a padded key, forward and backward
      unmasked_pad          one padded key (if there is one) keeps its logit 0 in the forward
      truncate_p            P truncated to bf16, forward and backward
      delta_rounded         delta = sum_d r(dout) r(out)
      no_scale_ds           ds = p (dp - delta)
      swap_dk_dv            the two key-side gradients exchanged
      skip_last_query_tile  the last 32-query tile is not accumulated into dK / dV
      lse_no_max            lse = log Z"""
    assert not set(defect) - set(DEFECTS), defect
    q, k, v, g = (rne_bf16(c[t]) for t in ("q", "k", "v", "dout"))
    G, n, dh = q.shape
    NP = 32 * -(-n // 32)
    kp, vp = np.zeros((G, NP, dh), F32), np.zeros((G, NP, dh), F32)
    kp[:, :n], vp[:, :n] = k, v
    sc = F32(c["scale"])
    s = q @ T(kp)
    masked = np.arange(NP) >= n
    bmask = masked.copy()
    if defect.get("drop_last_key"):
        masked[n - 1] = bmask[n - 1] = True
    if defect.get("unmasked_pad") and NP > n:
        masked[n] = False
    rp = trunc_bf16 if defect.get("truncate_p") else rne_bf16
    sm = np.where(masked, F32(-np.inf), s)
    mx = sm.max(-1, keepdims=True)
    with np.errstate(under="ignore", invalid="ignore"):
        pe = np.exp2((sm - mx) * F32(sc * LOG2E)).astype(F32)
    Z = pe.sum(-1, keepdims=True, dtype=F32)
    inv = F32(1) / Z
    out = ((rp(pe) @ vp) * inv).astype(F32)
    lse = (np.log(Z) if defect.get("lse_no_max") else sc * mx + np.log(Z)).astype(F32)[..., 0]
    res = {"out": out, "lse": lse}
    if want_probs:
        res["probs"] = (pe * inv)[:, :, :n]
    with np.errstate(all="ignore"):                                       # a defective lse overflows p: the checks see the inf / nan
        p = np.exp2(((sc * s - lse[..., None]) * LOG2E).astype(F32)).astype(F32)
        p[:, :, bmask] = 0
        do = np.asarray(c["dout"], F32)
        delta = ((g * rne_bf16(out)) if defect.get("delta_rounded") else (do * out)).sum(-1, keepdims=True, dtype=F32)
        ds = ((F32(1) if defect.get("no_scale_ds") else sc) * p * (g @ T(vp) - delta)).astype(F32)
        dsr, pr = rne_bf16(np.nan_to_num(ds, nan=np.nan, posinf=3e38, neginf=-3e38)), rp(np.minimum(p, F32(3e38)))
    rows = np.ones(n, bool)
    if defect.get("skip_last_query_tile"):
        rows[32 * ((n - 1) // 32):] = False
    with np.errstate(all="ignore"):
        dq = (dsr @ kp).astype(F32)
        dk = (T(dsr[:, rows]) @ q[:, rows]).astype(F32)[:, :n]
        dv = (T(pr[:, rows]) @ g[:, rows]).astype(F32)[:, :n]
    if defect.get("swap_dk_dv"):
        dk, dv = dv, dk
    res.update(dq=dq, dk=dk, dv=dv)
    return res
