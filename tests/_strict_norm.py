"""Strict instruments for the LayerNorm family (csrc/layernorm.hip) and the batch-moment / BatchNorm fold kernels (csrc/moments.hip):
case tables, float64 references, per-element bounds and numpy/float32 emulations of each kernel's contract with one defect switch
each.  Used by tests/test_strict_norm_gpu.py (the kernels) and tests/test_strict_norm_host.py (the CPU proof that the instruments
see each defect).  The shared pieces (bf, rng_of, check_exact, check_bound, check_bias, half_ulp_out, ops_bound, BIAS_*, SENTINEL)
are tests/_strict.py's.

LayerNorm bound.  u = 2^-24 (one fp32 rounding).  Per row, from the float64 reference: mean, d_i = x_i - mean, var = mean d_i^2,
s = sqrt(var + eps), A = mean |x_i|.  For ANY summation order (lanes, chunks, butterfly):

    e_mean   = (C - 1 + k_mean) u A           C - 1 adds; k_mean = 2 where the kernel multiplies by the rounded 1.0f / C (vec, add,
                                              slim), 1 where it divides by C (generic, patch merge: one correctly rounded division)
    e_d,i    = e_mean + u |d_i|               the subtraction
    e_var    = 2 e_mean mean|d_i| + e_mean^2 + (C + 4) u var
                                              d_i^2 with d_i off by e_d,i (first order 2 |d_i| e_d,i; the e_mean^2 term is what is left
                                              of it on a constant row, where every d_i is 0), the product, C - 1 adds, 1 / C
    rel_rstd = e_var / (2 s^2) + (2 R + 1) u  the add of eps (u of var + eps, halved by the root; counted whole) and rsqrtf to R ulp:
                                              an ulp is up to 2^-23 = 2 u of the value, so R ulp are 2 R u (the issue's starting
                                              point wrote R u; corrected here)
    pre_i    = |g_i| (e_d,i / s + (|d_i| / s) (rel_rstd + k_mul u)) + k_add u (|g_i d_i| / s + |b_i| + |res_i|)
    bound_i  = pre_i + half_ulp_out(|ref_i| + pre_i)

k_mul = 3, k_add = 2 for (x - mean) * rstd * g + b (+ res): d * rstd, * g and one spare on the product path (the subtraction's own
rounding is e_d,i's u |d_i|), + b and + res on the sums.  patch_merge_ln_kernel's epilogue is fmaf(v * rstd, g, b): k_mul = 2,
k_add = 1.  The compiler may contract a multiply and an add into one fma anywhere; that only removes roundings.

R: no document installed with the ROCm toolchain states an accuracy for rsqrtf, so R = 2 ulp is ASSUMED -- nobody has measured it.

Moments bound: out[c] = sum_rows (x - shift)^p is within (rows + 2) u sum |x - shift|^p in any order (the subtraction, the square
and rows - 1 adds; the fma of moments2 removes one).  Fold kernels: S.ops_bound with n_ops counted next to each formula below;
mv_bn_ema_fold1_fwd's variance carries the cancellation term 2 u (S2 / n + d^2) explicitly.
"""
from __future__ import annotations

import functools

import numpy as np

from tests import _strict as S
from tests._strict import BIAS_LIMIT, BIAS_MIN_ELEMS, SENTINEL, bf, check_bias, check_bound, check_exact, half_ulp_out, rng_of  # noqa: F401

F32, F64 = np.float32, np.float64
U = 2.0 ** -24
R_RSQRT = 2.0                 # ulp; assumed, not measured (module docstring)
GUARD = 64                    # tests/_slices.py
EPS = 1e-5
PAIRS = [("bf16", "bf16"), ("bf16", "fp32"), ("fp32", "bf16"), ("fp32", "fp32")]
EPC = {"bf16": 8, "fp32": 4}  # elements per 16-byte chunk


def q_of(dtype):
    return S.q_of(dtype)


# ================================================================================================ LayerNorm: launch shapes
def vec_shape(nch):
    """ln_vec_launch: (CHUNKS, WIDTH) for a row of nch 16-byte chunks."""
    if nch <= 16:
        return 1, 16
    if nch <= 32:
        return 1, 32
    for lim, ch in ((64, 1), (128, 2), (192, 3), (256, 4), (384, 6)):
        if nch <= lim:
            return ch, 64
    return 8, 64


def vec_blocks(nch, M):
    """Blocks of 4 waves ln_vec_launch starts, and the row groups they walk."""
    rpw = 64 // vec_shape(nch)[1]
    groups = -(-M // rpw)
    return min(-(-groups // 4), 2048), groups


def serves_slim(C, din, dout, gamma, beta, stride, flags):
    return (din == "fp32" and dout == "bf16" and gamma and beta and stride in (0, C) and C % 256 == 0 and C <= 768
            and "no_ln_slim" not in flags and "force_generic" not in flags)


def route(C, din, dout, gamma, beta, stride, flags):
    """mv_layernorm_fwd's routing, restated: the kernel name a call must reach."""
    if serves_slim(C, din, dout, gamma, beta, stride, flags):
        return "layernorm_slim"
    epc = EPC[din]
    if C % epc == 0 and (stride or C) % epc == 0 and C // epc <= 64 * 8 and "force_generic" not in flags:
        return "layernorm_vec"
    return "layernorm"


class LnCase:
    """One mv_layernorm_fwd case.  kind: gauss | offset (mean 4096, sigma 1) | small (sigma 0.01) | const (0.3 everywhere)."""

    def __init__(self, M, C, din, dout, expect, gamma=True, beta=True, stride=0, flags=(), kind="gauss", note=""):
        self.M, self.C, self.din, self.dout, self.expect = M, C, din, dout, expect
        self.gamma, self.beta, self.stride, self.flags, self.kind, self.note = gamma, beta, stride, tuple(flags), kind, note
        self.nch = C // EPC[din]
        if expect == "layernorm_vec":
            self.geom = ("vec", EPC[din]) + vec_shape(self.nch)
            shape = "ch%dw%d" % vec_shape(self.nch)
            self.id = f"nch{self.nch}_{shape}_M{M}_{din}_{dout}"
        elif expect == "layernorm_slim":
            self.geom = ("slim", 4, C // 256, 64)
            self.id = f"slim_C{C}_M{M}"
        else:
            self.geom = ("generic", 1, -(-C // 64), 64)
            self.id = f"generic_C{C}_M{M}_{din}_{dout}"
        if not gamma or not beta:
            self.id += "_" + ("g" if gamma else "") + ("b" if beta else "") + ("none" if not (gamma or beta) else "_only")
        if note:
            self.id += "_" + note
        self.k_mean = 1 if expect == "layernorm" else 2

    @property
    def xs(self):
        return self.stride or self.C


VEC_NCH = [13, 16, 24, 33, 64, 65, 129, 193, 257, 385, 512]


def _vec_case(nch, M, din, dout, **kw):
    C = nch * EPC[din]
    flags = tuple(kw.pop("flags", ()))
    if serves_slim(C, din, dout, kw.get("gamma", True), kw.get("beta", True), kw.get("stride", 0), flags):
        flags += ("no_ln_slim",)          # nch 64 fp32 -> bf16 is the slim kernel's C = 256: the flag keeps the case on layernorm_vec
    return LnCase(M, C, din, dout, "layernorm_vec", flags=flags, **kw)


def _build_ln_cases():
    vec = [_vec_case(nch, 37, di, do) for nch in VEC_NCH for di, do in PAIRS]
    for nch in (13, 65):
        for M in (1, 64 // vec_shape(nch)[1] + 1):
            vec += [_vec_case(nch, M, di, do) for di, do in PAIRS]
    for nch in (24, 129):
        for g, b in ((True, False), (False, True), (False, False)):
            vec += [_vec_case(nch, 37, di, do, gamma=g, beta=b) for di, do in PAIRS]
    vec.append(_vec_case(33, 37, "bf16", "bf16", stride=33 * 8 + 16, note="strided"))
    vec.append(_vec_case(8, 65937, "fp32", "fp32", note="gridstride"))            # C = 32 fp32: WIDTH 16, 16485 row groups
    vec.append(_vec_case(33, 16485, "bf16", "bf16", note="gridstride"))           # C = 264 bf16: WIDTH 64
    vec.append(_vec_case(32, 37, "fp32", "fp32", kind="offset", note="offset4096"))
    vec.append(_vec_case(13, 37, "fp32", "fp32", kind="small", note="sigma0.01"))  # var = 10 eps: where eps sits decides the result
    vec.append(_vec_case(13, 37, "bf16", "bf16", kind="const", note="const"))
    vec.append(_vec_case(65, 37, "fp32", "fp32", kind="const", note="const"))
    # C = 20 fp32 is five whole chunks: layernorm_vec serves it (WIDTH 16, eleven dead lanes); C = 22 is the generic kernel's
    vec.append(_vec_case(5, 7, "fp32", "fp32", note="C20"))
    gen = [LnCase(7, 22, "fp32", "fp32", "layernorm"), LnCase(7, 70, "bf16", "bf16", "layernorm"),
           LnCase(7, 3072, "fp32", "fp32", "layernorm"),
           LnCase(37, 65 * 8, "bf16", "bf16", "layernorm", flags=("force_generic",), note="forced"),
           LnCase(7, 264, "bf16", "bf16", "layernorm", stride=264 + 3, note="stride_C+3")]
    slim = [LnCase(5, C, "fp32", "bf16", "layernorm_slim") for C in (256, 512, 768)]
    slim.append(LnCase(8195, 256, "fp32", "bf16", "layernorm_slim", note="gridstride"))
    unslim = [LnCase(c.M, c.C, "fp32", "bf16", "layernorm_vec", flags=("no_ln_slim",), note="no_ln_slim") for c in slim]
    not_slim = [LnCase(5, 1024, "fp32", "bf16", "layernorm_vec", note="C1024_not_slim")]
    return vec, gen, slim, unslim + not_slim


LN_VEC, LN_GENERIC, LN_SLIM, LN_UNSLIM = _build_ln_cases()
LN_CASES = LN_VEC + LN_GENERIC + LN_SLIM + LN_UNSLIM
assert len({c.id for c in LN_CASES}) == len(LN_CASES)


def affine_of(C, gamma=True, beta=True, seed=71):
    rng = rng_of(seed + C)
    g = S.gauss_scale(rng, C) if gamma else None
    b = rng.standard_normal(C).astype(F32) if beta else None
    return g, b


def rows_data(M, C, dtype, kind="gauss", seed=70):
    """(M, C) rows rounded to the storage type: unit-variance Gaussian rows about a per-row mean in [-1, 1]."""
    rng = rng_of(seed + 7 * C + M % 1000)
    if kind == "const":
        return q_of(dtype)(np.full((M, C), 0.3))
    if kind == "small":
        return q_of(dtype)(0.01 * rng.standard_normal((M, C)))
    if kind == "offset":
        return q_of(dtype)(4096.0 + rng.standard_normal((M, C)))
    return q_of(dtype)(rng.standard_normal((M, C), dtype=F32) + rng.uniform(-1.0, 1.0, (M, 1)).astype(F32))


def rep_rows(M, C, dtype, seed=72):
    """Row-position invariance and isolation in one input: three base rows in a fixed shuffled order over the M rows, and one row of
    NaN in the middle.  Returns (x, idx (M,) with -1 at the NaN row)."""
    rng = rng_of(seed + 3 * C + M % 1000)
    base = rows_data(3, C, dtype, seed=seed)
    idx = rng.integers(0, 3, M)
    idx[:min(3, M)] = (0, 1, 2)[:M]
    x = base[idx % 3].copy()
    if M >= 3:
        nan_row = M // 2
        x[nan_row] = np.nan
        idx[nan_row] = -1
    return x, idx


def strided(x, xs):
    """x (M, C) laid out with row stride xs, NaN in the gap columns."""
    M, C = x.shape
    full = np.full((M, xs), np.nan, F32)
    full[:, :C] = x
    return full


@functools.lru_cache(maxsize=None)
def ln_case_data(i):
    c = LN_CASES[i]
    x = rows_data(c.M, c.C, c.din, c.kind)
    g, b = affine_of(c.C, c.gamma, c.beta)
    ref, bound = ln_ref_bound(x, g, b, None, EPS, c.dout, k_mean=c.k_mean)
    for a in (x, ref, bound):
        a.setflags(write=False)
    return c, x, g, b, ref, bound


# ================================================================================================ LayerNorm: reference and bound
def ln_ref_bound(x, gamma, beta, res, eps, out, k_mean=2, k_mul=3, k_add=2, R=R_RSQRT):
    """float64 LayerNorm of the rows of x (+ res) and the per-element bound of the module docstring.  A row with a NaN gives NaN."""
    x = np.asarray(x, F64)
    C = x.shape[-1]
    eps = float(F32(eps))
    g = np.ones(C) if gamma is None else np.asarray(gamma, F64)
    b = np.zeros(C) if beta is None else np.asarray(beta, F64)
    r = np.zeros_like(x) if res is None else np.asarray(res, F64)
    with np.errstate(invalid="ignore"):
        mean = x.mean(-1, keepdims=True)
        d = x - mean
        var = (d * d).mean(-1, keepdims=True)
        s = np.sqrt(var + eps)
        ref = r + (d / s * g + b)
        A = np.abs(x).mean(-1, keepdims=True)
        e_mean = (C - 1 + k_mean) * U * A
        e_d = e_mean + U * np.abs(d)
        e_var = 2.0 * e_mean * np.abs(d).mean(-1, keepdims=True) + e_mean ** 2 + (C + 4) * U * var
        rel_rstd = e_var / (2.0 * s * s) + (2.0 * R + 1.0) * U
        pre = np.abs(g) * (e_d / s + np.abs(d) / s * (rel_rstd + k_mul * U)) + k_add * U * (np.abs(g * d) / s + np.abs(b) + np.abs(r))
        ok = np.isfinite(ref)
        bound = pre + half_ulp_out(np.where(ok, np.abs(ref) + pre, 0.0), out)
    return ref, bound


# ================================================================================================ LayerNorm: emulation
LN_DEFECTS = ("one_pass", "no_eps", "eps_outside", "c_minus_1", "dead_chunk", "prev_subrow", "store_clamped", "gb_late")


def _butterfly(v, width):
    idx = np.arange(width)
    o = width // 2
    while o > 0:
        v = v + v[:, idx ^ o]
        o >>= 1
    return v[:, 0]


def _rsqrt32(v):
    with np.errstate(divide="ignore", invalid="ignore"):
        return (1.0 / np.sqrt(np.asarray(v, F32).astype(F64))).astype(F32)


def _row_stats(x, N, CHUNKS, WIDTH, eps, div=False, pairwise=False, defect=None):
    """(mean, rstd) per row as WIDTH lanes compute them: lane sl holds chunk sl + WIDTH i (clamped to the last chunk and masked out
    when past it), adds its values in order (pairwise: (x + y) + (z + w) per float4), then the xor butterfly; two passes."""
    M, C = x.shape
    nch = C // N
    assert nch * N == C, "rows are whole chunks"
    c = np.arange(WIDTH)[None, :] + WIDTH * np.arange(CHUNKS)[:, None]
    on = c < nch
    a = x.reshape(M, nch, N)[:, np.minimum(c, nch - 1)]                  # (M, CHUNKS, WIDTH, N)
    cnt = np.ones_like(on) if defect == "dead_chunk" else on
    zero = F32(0)

    def lane_sum(v, mask):
        s = np.zeros((M, WIDTH), F32)
        for i in range(CHUNKS):
            if pairwise:
                s = s + np.where(mask[i], (v[:, i, :, 0] + v[:, i, :, 1]) + (v[:, i, :, 2] + v[:, i, :, 3]), zero)
            else:
                for e in range(N):
                    s = s + np.where(mask[i], v[:, i, :, e], zero)
        return _butterfly(s, WIDTH)

    Cf = F32(C)
    invC = F32(1) / Cf
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        tot = lane_sum(a, cnt)
        mean = tot / Cf if div else tot * invC
        if defect == "one_pass":
            var = lane_sum(a * a, on) * invC - mean * mean
        else:
            d = a - mean[:, None, None, None]
            q = lane_sum(d * d, on)
            if defect == "c_minus_1":
                var = q * (F32(1) / F32(C - 1))
            else:
                var = q / Cf if div else q * invC
        e = F32(eps)
        if defect == "no_eps":
            rstd = _rsqrt32(var)
        elif defect == "eps_outside":
            rstd = (F32(1) / (np.sqrt(var) + e)).astype(F32)
        else:
            rstd = _rsqrt32(var + e)
    return mean.astype(F32), rstd


def _late(p, N):
    """gamma / beta read one chunk late (clamped at the last chunk)."""
    nch = p.size // N
    return p.reshape(nch, N)[np.minimum(np.arange(nch) + 1, nch - 1)].reshape(-1)


def emu_layernorm(x, gamma, beta, eps, out, geom, defect=None, store_mode="rne"):
    """mv_layernorm_fwd's three kernels in float32: geom = (kind, N, CHUNKS, WIDTH), kind vec | slim | generic.  Returns (y (M, C),
    guard (GUARD,)): the guard holds the sentinel unless defect == "store_clamped" (the re-read rows past M of the last row group
    store too).  One defect of LN_DEFECTS at a time; store_mode="trunc" is the truncating bf16 store."""
    kind, N, CHUNKS, WIDTH = geom
    x = np.asarray(x, F32)
    M, C = x.shape
    mean, rstd = _row_stats(x, N, CHUNKS, WIDTH, eps, div=kind == "generic", pairwise=kind == "slim", defect=defect)
    rpw = 64 // WIDTH
    if defect == "prev_subrow":
        r = np.arange(M)
        src = np.where(r % rpw != 0, r - 1, r)
        mean, rstd = mean[src], rstd[src]
    g = np.ones(C, F32) if gamma is None else np.asarray(gamma, F32)
    b = np.zeros(C, F32) if beta is None else np.asarray(beta, F32)
    if defect == "gb_late":
        g, b = _late(g, N), _late(b, N)
    with np.errstate(invalid="ignore", over="ignore"):
        y = S.store((x - mean[:, None]) * rstd[:, None] * g + b, out, store_mode)
    guard = np.full(GUARD, SENTINEL, F32)
    if defect == "store_clamped":
        extra = -(-M // rpw) * rpw - M
        spill = np.tile(y[M - 1], extra)[:GUARD]
        guard[:spill.size] = spill
    return y, guard


def emu_layernorm_add(z, res, gamma, beta, eps, lo, geom, defect=None):
    """layernorm_add_kernel: (y fp32, y_lo rounded ONCE from the same fp32 row, or None)."""
    _, N, CHUNKS, WIDTH = geom
    z = np.asarray(z, F32)
    mean, rstd = _row_stats(z, N, CHUNKS, WIDTH, eps, defect=defect)
    with np.errstate(invalid="ignore"):
        o = (z - mean[:, None]) * rstd[:, None] * np.asarray(gamma, F32) + np.asarray(beta, F32)
        if res is not None:
            o = np.asarray(res, F32) + o
    return o, (None if lo is None else S.store(o, lo))


def merge_rows(x):
    """(B, H, W, C) -> (B Ho Wo, 4 C): [x[0::2, 0::2], x[1::2, 0::2], x[0::2, 1::2], x[1::2, 1::2]] along the channel."""
    m = np.concatenate([x[:, 0::2, 0::2], x[:, 1::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 1::2]], -1)
    return m.reshape(-1, m.shape[-1])


def emu_patch_merge_ln(x, gamma, beta, eps, out, swap12=False, store_mode="rne"):
    """patch_merge_ln_kernel: the gather, pairwise float4 sums over NV float4 per lane, s / (4 C), fmaf(v * rstd, g, b)."""
    x = np.asarray(x, F32)
    C = x.shape[-1]
    rows = merge_rows(x)
    if swap12:
        rows = np.concatenate([rows[:, :C], rows[:, 2 * C:3 * C], rows[:, C:2 * C], rows[:, 3 * C:]], -1)
    nv = pm_nv(C)
    mean, rstd = _row_stats(rows, 4, nv, 64, eps, div=True, pairwise=True)
    v = (rows - mean[:, None]) * rstd[:, None]
    y = (v.astype(F64) * np.asarray(gamma, F32).astype(F64) + np.asarray(beta, F32).astype(F64)).astype(F32)      # fmaf
    return S.store(y, out, store_mode)


def pm_nv(C):
    nv = (C + 63) // 64
    return 2 if nv <= 2 else (3 if nv <= 3 else 6)


def pm_data(B, H, W, C, seed=73):
    """fp32 map whose four gathered pixels have the means 0, 2, 4, 6 (segment = (h & 1) + 2 (w & 1)); gamma, beta over 4 C."""
    rng = rng_of(seed + C)
    x = rng.standard_normal((B, H, W, C))
    x = x + 2.0 * ((np.arange(H) & 1)[None, :, None, None] + 2 * (np.arange(W) & 1)[None, None, :, None])
    g, b = affine_of(4 * C, seed=seed)
    return x.astype(F32), g, b


PM_CASES = [(2, 4, 6, C) for C in (16, 20, 100, 128, 132, 192, 196, 384)]
PM_GRIDSTRIDE = (1, 182, 182, 16)


# ------------------------------------------------------------------------------------------------ mv_layernorm_add_fwd cases
ADD_CASES = [(nch, zd, res, lo) for nch in (13, 65, 385) for zd in ("bf16", "fp32") for res in (True, False)
             for lo in (None, "bf16", "fp32")]
ADD_GRIDSTRIDE = (16485, 264, "bf16", True, "bf16")


@functools.lru_cache(maxsize=None)
def add_data(M, C, zd, with_res):
    z = rows_data(M, C, zd, seed=74)
    res = rng_of(75 + C).standard_normal((M, C)).astype(F32) if with_res else None
    g, b = affine_of(C, seed=76)
    ref, bound = ln_ref_bound(z, g, b, res, EPS, "fp32")
    return z, res, g, b, ref, bound


def rows_equal(got, idx):
    """Row-position invariance: rows with the same base index must be bitwise equal.  Returns the number of rows that differ."""
    got = np.ascontiguousarray(np.asarray(got, F32)).view(np.uint32)
    bad = 0
    for k in range(3):
        rows = np.nonzero(idx == k)[0]
        if rows.size > 1:
            bad += int((got[rows] != got[rows[0]]).any(axis=1).sum())
    return bad


# ================================================================================================ moments
MOM_BLOCKS = 1024
MOM_CASES = [(1, 8), (300, 8), (5000, 8), (200, 24), (1000, 96), (23189, 96), (37, 1032), (1, 2040), (37, 2040), (1, 2048),
             (37, 2048), (1107, 2048)]
MOM_CAP = (16384, 2048)       # bf16 only: the smallest row count that reaches the cap of 1024 blocks (64 MB)


def mom_geometry(rows, C):
    """mv_channel_moments_fwd's arithmetic: (V, RS, idle threads, G, rows of the grid per step)."""
    V = C >> 3
    RS = 256 // V
    need = -(-rows // (16 * RS))
    G = min(need, MOM_BLOCKS)
    return V, RS, 256 - RS * V, G, G * RS


def mom_data(rows, C, dtype, kind, shift_sigmas=0.3, seed=80):
    """kind "int": integer shift in [-8, 8], x = shift + integers in [-16, 16].  kind "gauss": x ~ N(mean_c, sigma_c), shift at
    `shift_sigmas` standard deviations from the batch mean (alternating sides)."""
    rng = rng_of(seed + C + rows % 997)
    if kind == "int":
        shift = rng.integers(-8, 9, C).astype(F32)
        x = shift[None, :] + rng.integers(-16, 17, (rows, C), dtype=np.int8).astype(F32)
        return x, shift
    mu, sg = rng.uniform(-2.0, 2.0, C), rng.uniform(0.5, 2.0, C)
    x = q_of(dtype)(rng.standard_normal((rows, C), dtype=F32) * sg.astype(F32) + mu.astype(F32))
    side = np.where(np.arange(C) % 2 == 0, 1.0, -1.0)
    shift = (x.astype(F64).mean(0) + side * shift_sigmas * sg).astype(F32)
    return x, shift


def mom_ref(x, shift, p):
    """(float64 sum over the rows of (x - shift)^p, the same sum of |x - shift|^p), in slabs of rows to bound the memory."""
    rows, C = x.shape
    sh = np.zeros(C) if shift is None else np.asarray(shift, F64)
    ref, mag = np.zeros(C), np.zeros(C)
    for r0 in range(0, rows, 4096):
        d = x[r0:r0 + 4096].astype(F64) - sh
        ref += (d ** p).sum(0)
        mag += (np.abs(d) ** p).sum(0)
    return ref, mag


def mom_bound(rows, mag):
    return (rows + 2) * U * np.asarray(mag, F64)


def prove_mom_exact(name, x, shift, rows):
    """The exact instrument's preconditions: integers, |x - shift| <= 16, x exact in bf16, every partial sum below 2^24."""
    d = x.astype(F64) - (0.0 if shift is None else shift.astype(F64))
    assert np.array_equal(np.rint(x), x) and float(np.abs(x).max()) <= S.BF16_INT_MAX, name
    assert shift is None or np.array_equal(np.rint(shift), shift), name
    assert float(np.abs(d).max()) <= (16 if shift is not None else 24), name
    assert 24 * 24 * rows < S.ACC_INT_MAX, f"{name}: {rows} rows of squares up to 576 reach 2^24"


MOM_DEFECTS = ("tail_skip", "double_count", "read_past_G", "square_first")


def emu_moments(x, shift, mode, defect=None):
    """moments_partial_kernel / moments2_partial_kernel + moments_final_kernel in float32.  mode "sum" | "sq" | "both" (moments2: the
    sums and, by fma, the squares, 2 C outputs).  Slot p = block * RS + rs of the grid takes the rows p, p + step, ...: n of them, the
    first 4 (n / 4) in the unrolled loop, the rest in the tail.  The workspace holds NaN where no block wrote.  Defects:
      tail_skip      the tail starts one step late (its first row is lost)
      double_count   the tail starts one step early (the unrolled loop's last row is counted again)
      read_past_G    the final kernel adds partial G as well
      square_first   d = x^2 - shift instead of (x - shift)^2"""
    x = np.asarray(x, F32)
    rows, C = x.shape
    V, RS, _, G, step = mom_geometry(rows, C)
    sh = np.zeros(C, F32) if shift is None else np.asarray(shift, F32)
    K = -(-rows // step)
    p = np.arange(step)
    n = np.where(p < rows, -(-(rows - p) // step), 0)
    k = np.arange(K)[:, None]
    w = (k < n[None, :]).astype(F32)
    head = 4 * (n // 4)
    if defect == "tail_skip":
        w[(k == head[None, :]) & (head < n)[None, :]] = 0
    if defect == "double_count":
        w[(k == head[None, :] - 1) & (head >= 4)[None, :]] = 2
    pad = np.zeros((K * step, C), F32)
    pad[:rows] = x
    pad = pad.reshape(K, step, C)
    a1, a2 = np.zeros((step, C), F32), np.zeros((step, C), F32)
    for kk in range(K):
        wk = w[kk][:, None]
        live, xk = wk != 0, pad[kk]
        d = np.where(live, xk - sh, F32(0))
        sq = np.where(live, xk * xk - sh, F32(0)) if defect == "square_first" else d * d
        if mode in ("sum", "both"):
            a1 = a1 + d * wk
        if mode == "sq":
            a2 = a2 + sq * wk
        elif mode == "both":
            sq64 = sq.astype(F64) if defect == "square_first" else d.astype(F64) * d.astype(F64)
            a2 = (sq64 * wk + a2.astype(F64)).astype(F32)                                # fmaf(d, d, a2)
    acc = {"sum": a1, "sq": a2, "both": np.concatenate([a1, a2], 1)}[mode]
    Cw = acc.shape[1]
    acc = acc.reshape(G, RS, Cw)
    part = np.zeros((G, Cw), F32)
    for j in range(RS):
        part = part + acc[:, j]
    ws = np.full((MOM_BLOCKS + 1, Cw), np.nan, F32)
    ws[:G] = part
    Gr = G + 1 if defect == "read_past_G" else G
    out = np.zeros(Cw, F32)
    for qq in range(16):
        s = np.zeros(Cw, F32)
        for g in range(qq, Gr, 16):
            s = s + ws[g]
        out = out + s
    return out


# ================================================================================================ BatchNorm fold kernels
def fold_data(C, seed=90):
    """Per-channel batch statistics of n = 1568 rows and the running values before the call (all fp32)."""
    rng = rng_of(seed + C)
    n = 1568.0
    mean = rng.uniform(-2.0, 2.0, C).astype(F32)
    var = rng.uniform(0.25, 4.0, C).astype(F32)
    d = {"n": n, "sum": (mean.astype(F64) * n).astype(F32), "mean": mean, "sqdev": (var.astype(F64) * n).astype(F32),
         "run_mean": rng.uniform(-2.0, 2.0, C).astype(F32), "run_var": rng.uniform(0.25, 4.0, C).astype(F32),
         "weight": S.gauss_scale(rng, C), "bias": rng.standard_normal(C).astype(F32), "momentum": F32(0.99), "eps": F32(1e-5)}
    # single-pass sums about shift = run_mean: d = mean - run_mean, S1 = n d, S2 = n (var + d^2)
    dd = mean.astype(F64) - d["run_mean"].astype(F64)
    d["sums"] = np.concatenate([n * dd, n * (var.astype(F64) + dd * dd)]).astype(F32)
    return d


def const_sums(C, n=1568.0, seed=91):
    """sums of a CONSTANT input x = shift + d0 per channel: S1 = n d0, S2 = n d0^2 (each rounded to fp32).  The variance is 0; the
    fp32 S2 / n - d^2 is a rounding residue of either sign."""
    d0 = rng_of(seed + C).uniform(-3.0, 3.0, C)
    return np.concatenate([n * d0, n * d0 * d0]).astype(F32), d0


def bn_mean_ref(sum_, n):
    """mean = sum / n: one rounding (n_ops = 1)."""
    ref = np.asarray(sum_, F64) / float(n)
    return ref, np.abs(ref), 1


def fold_ref(sqdev, mean, n, run_mean, run_var, weight, bias, momentum, eps, first_time):
    """float64 bn_ema_fold_kernel and (mag, n_ops) per output for S.ops_bound (one op = 2^-23 of mag, as everywhere in _strict.py):
      run_mean   first call: a copy (0).  else (1 - m) [1], * mean [1], m * run_mean [1], the add [1]: 4 of |(1-m) mean| + |m run_mean|
      run_var    the division [1] and the same four: 5 of (1 - m) var + m run_var (first call: 1)
      scale      rv + eps [1], sqrtf [1], 1 / (.) [1], weight * inv [1], and rv's relative error halved by the square root
                 (all terms of rv are positive, so its 5 operations are relative to rv itself: 2.5 -> 3): 7 of |scale|
      shift      bias - rm * scale: rm's 4 (of mag_rm |scale|), scale's 7, the product [1], the difference [1]: 13 of mag_rm |scale| + |bias|"""
    m, e = float(F32(momentum)), float(F32(eps))
    C = np.asarray(mean).size
    w = np.ones(C) if weight is None else np.asarray(weight, F64)
    b = np.zeros(C) if bias is None else np.asarray(bias, F64)
    var = np.asarray(sqdev, F64) / float(n)
    mean = np.asarray(mean, F64)
    if first_time:
        rm, rv, mag_rm, mag_rv, n_rm, n_rv = mean, var, np.abs(mean), var, 0, 1
    else:
        rm = (1.0 - m) * mean + m * np.asarray(run_mean, F64)
        rv = (1.0 - m) * var + m * np.asarray(run_var, F64)
        mag_rm = np.abs((1.0 - m) * mean) + np.abs(m * np.asarray(run_mean, F64))
        mag_rv, n_rm, n_rv = rv, 4, 5
    sc = w / np.sqrt(rv + e)
    sh = b - rm * sc
    return {"run_mean": (rm, mag_rm, n_rm), "run_var": (rv, mag_rv, n_rv), "scale": (sc, np.abs(sc), 7),
            "shift": (sh, mag_rm * np.abs(sc) + np.abs(b), 13)}


def fold1_ref(sums, n, run_mean, run_var, weight, bias, momentum, eps):
    """float64 bn_ema_fold1_kernel and an explicit bound per output, in u = 2^-24, every magnitude from the float64 values:
      d = S1 / n [u |d|];  q = S2 / n [u q];  d * d [2 u d^2 from d, u d^2 its own];  q - d d [u |var|]:
          e_var = 2 u (q + d^2) + u (d^2 + var)         the first term IS the cancellation: it is relative to q + d^2, not to var, and
                                                        grows as 1 + 2 (mean - shift)^2 / sigma^2 against var (fmaxf(., 0) is exact
                                                        and 1-Lipschitz, the reference variance is >= 0)
      mean = run_mean + d:  e_m = u |d| + u |mean|
      rm = (1 - m) mean + m run_mean:  e_rm = (1 - m) e_m + 4 u mag_rm,   mag_rm = |(1 - m) mean| + |m run_mean|   (1 - m, two products, add)
      rv likewise:          e_rv = (1 - m) e_var + 4 u mag_rv
      scale = weight / sqrt(rv + eps):  rel = (e_rv + u (rv + eps)) / (2 (rv + eps)) + 3 u   (sqrtf, the division, the product)
      shift = bias - rm scale:  |scale| e_rm + |rm scale| rel + u |rm scale| + u (|bias| + |rm scale|)
    each plus half an fp32 ulp of the result."""
    m, e, n = float(F32(momentum)), float(F32(eps)), float(n)
    sums = np.asarray(sums, F64)
    C = sums.size // 2
    w = np.ones(C) if weight is None else np.asarray(weight, F64)
    b = np.zeros(C) if bias is None else np.asarray(bias, F64)
    rm0, rv0 = np.asarray(run_mean, F64), np.asarray(run_var, F64)
    d, q = sums[:C] / n, sums[C:] / n
    var = np.maximum(q - d * d, 0.0)
    e_var = 2.0 * U * (q + d * d) + U * (d * d + var)
    mean = rm0 + d
    e_m = U * np.abs(d) + U * np.abs(mean)
    rm = (1.0 - m) * mean + m * rm0
    mag_rm = np.abs((1.0 - m) * mean) + np.abs(m * rm0)
    e_rm = (1.0 - m) * e_m + 4.0 * U * mag_rm
    rv = (1.0 - m) * var + m * rv0
    e_rv = (1.0 - m) * e_var + 4.0 * U * ((1.0 - m) * var + m * np.abs(rv0))
    rel = (e_rv + U * (rv + e)) / (2.0 * (rv + e)) + 3.0 * U
    sc = w / np.sqrt(rv + e)
    sh = b - rm * sc
    e_sc = np.abs(sc) * rel
    e_sh = np.abs(sc) * e_rm + np.abs(rm * sc) * rel + U * np.abs(rm * sc) + U * (np.abs(b) + np.abs(rm * sc))

    def fin(ref, err):
        return ref, err + half_ulp_out(np.abs(ref) + err, "fp32")
    return {"run_mean": fin(rm, e_rm), "run_var": fin(rv, e_rv), "scale": fin(sc, e_sc), "shift": fin(sh, e_sh)}


def emu_bn_mean(sum_, n):
    return np.asarray(sum_, F32) / F32(n)


def _fold_tail(rm, rv, weight, bias, eps):
    C = rm.size
    inv = F32(1) / np.sqrt(rv + F32(eps))
    sc = (np.ones(C, F32) if weight is None else np.asarray(weight, F32)) * inv
    sh = (np.zeros(C, F32) if bias is None else np.asarray(bias, F32)) - rm * sc
    return {"run_mean": rm, "run_var": rv, "scale": sc.astype(F32), "shift": sh.astype(F32)}


def emu_fold(sqdev, mean, n, run_mean, run_var, weight, bias, momentum, eps, first_time):
    m = F32(momentum)
    var = np.asarray(sqdev, F32) / F32(n)
    rm, rv = np.asarray(mean, F32), var
    if not first_time:
        rm = (F32(1) - m) * rm + m * np.asarray(run_mean, F32)
        rv = (F32(1) - m) * rv + m * np.asarray(run_var, F32)
    return _fold_tail(rm, rv, weight, bias, eps)


def emu_fold1(sums, n, run_mean, run_var, weight, bias, momentum, eps, clamp=True):
    """clamp=False: the defect `fmaxf(., 0) removed`."""
    m = F32(momentum)
    sums = np.asarray(sums, F32)
    C = sums.size // 2
    d = sums[:C] / F32(n)
    var = sums[C:] / F32(n) - d * d
    if clamp:
        var = np.maximum(var, F32(0))
    rm0 = np.asarray(run_mean, F32)
    mean = rm0 + d
    rm = (F32(1) - m) * mean + m * rm0
    rv = (F32(1) - m) * var + m * np.asarray(run_var, F32)
    with np.errstate(invalid="ignore"):
        return _fold_tail(rm, rv, weight, bias, eps)


# ================================================================================================ the two judgements both modules use
def judge(got, ref, bound, out):
    """(bound info, bias info): every element within `bound`; the project's bias rule where it applies -- a bf16 output with at least
    BIAS_MIN_ELEMS reference elements of |ref| >= 2^-6, decided from the reference alone."""
    a = check_bound(got, ref, None, 0, out, bound=bound)
    applies = out == "bf16" and int((np.abs(ref) >= 2.0 ** -6).sum()) >= BIAS_MIN_ELEMS
    b = check_bias(got, ref, out) if applies else {"ok": True, "bias": float("nan"), "n_bias": 0}
    return a, b


def judge_rep(got, idx, ref, bound, out):
    """The rep_rows input: the NaN row gives NaN, every other row is finite, inside the bound and bitwise equal to the rows of the
    same base.  Returns the list of what failed (empty: passed)."""
    got = np.asarray(got, F64)
    keep = idx >= 0
    bad = []
    if (~keep).any() and not np.isnan(got[~keep]).all():
        bad.append("the NaN row came out finite")
    if not np.isfinite(got[keep]).all():
        bad.append(f"{int((~np.isfinite(got[keep])).any(axis=1).sum())} other rows are not finite")
    else:
        a = check_bound(got[keep], ref[keep], None, 0, out, bound=bound[keep])
        if not a["ok"]:
            bad.append(f"bound: {a}")
    n = rows_equal(got[keep].astype(F32), idx[keep])
    if n:
        bad.append(f"{n} rows differ bitwise from an equal input row elsewhere")
    return bad
