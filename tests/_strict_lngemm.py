"""Strict instruments for the GEMM kernels that normalise their rows on the way in: mv_ln_linear_fwd (csrc/stream1x1.hip, LN mode),
mv_ln_mlp_fwd / mv_ln_mlp_res_fwd (csrc/ln_mlp.hip) and mv_ln_mlp_stream_fwd / mv_ln_mlp_stream_res_fwd (csrc/ln_mlp_stream.hip).
Case tables, data builders, CPU proofs, float64 references with per-element bounds, and numpy/float32 emulations of each kernel's
order of operations with one defect switch each.  Used by tests/test_strict_lngemm_gpu.py (the kernels) and
tests/test_strict_lngemm_host.py (the CPU proof that the instruments see each defect).  The shared pieces are tests/_strict.py's and
tests/_strict_norm.py's.

Instrument 1 -- exact through the LayerNorm.  The three kernels compute (x - mean) * rstd in fp32 and round it to bf16 straight into
the MFMA fragment (pack_bf2).  Rows are m_r +- a_r: half the entries +, half -, a_r a power of two >= 1/4, m_r an integer multiple
of a_r with |m_r| <= 64 a_r (the builders keep to 8 a_r), every entry representable in the stream dtype, a sign pattern per row.
The true normalised value is +- a / sqrt(a^2 + eps); `prove_pm1` asserts in float64, row by row, that it is within 2^-10 of +-1 and
that the whole fp32 error ln_ref_bound allows (any summation order, rsqrtf to R ulp) keeps it strictly inside (1 - 2^-9, 1 + 2^-8),
the interval bf16 rounds to 1.  The fragment therefore holds exactly +-1.0 and, with integer weights, every later sum is an exact
integer: the output must EQUAL the float64 reference (S.prove_exact asserts the rest: magnitudes, used reduction indices, non-zero
outputs).  Neighbouring rows (m ^ 1 and m +- 1) differ by a factor >= 4 in a_r, so a row normalised with a neighbour's statistics
comes out as +-4 or +-1/4, never +-1.
  ln_mlp chain.  gelu_tanh_f / gelu_tanh_pack2 (csrc/common.h) are x * rcp(1 + exp2(t)), t = x (k0 + k1 x^2) with the float constants
  k0 = -2 sqrt(2/pi) log2(e), k1 = k0 * 0.044715f.  `gelu_exact_from()` finds, in float32 arithmetic, the smallest |x| at which
  |t| > 128 (10.06...).  From the source: for x at or above it t < -128, exp2(t) < 2^-128 < 2^-25 and 1 + exp2(t) rounds to 1 whatever
  exp2 returns there (0, a subnormal, or anything below 2^-25); for x at or below minus it t > 128 and exp2(t) overflows to +inf,
  1 + inf = inf, rcp(inf) = 0 and x * 0 = -0 (IEEE special values).  At x = 0, t = 0 and the result is 0 * rcp(1 + exp2(0)).
  SUPPOSED, not in the source: v_rcp_f32(1) = 1, v_rcp_f32(2) = 0.5, v_exp_f32(0) = 1 (v_exp_f32(+-0)).  With fc1 entries in
  {-16, 0, 16} gamma (gamma in {1, 2}) and b1' a multiple of 16 every pre-activation is a multiple of 16: GELU acts as an exact ReLU.
  fc2 has entries in {-1, 0, 1} and an integer bias; hidden values and outputs stay bf16-exact multiples of 16 where bf16 holds them.

Instrument 2 -- per-element bound on Gaussian rows (per-row scale and offset, every seventh row with a common offset of 50 of its
standard deviations, row 5 constant: variance 0, reference output b' exactly).  The reference is float64 ON THE OPERANDS THE KERNEL
GETS: the bf16-rounded folded weights, the fp32 folded biases.  With u23 = 2^-23 and everything from float64 values:
    n, e_ln        = _strict_norm.ln_ref_bound(x, no affine, bf16 output)          per element, the pack's half ulp included
    p              = n W'^T + b'                   E1 = e_ln |W'|^T                 mag1 = (|n| + e_ln) |W'|^T + |b'|
    e_p            = E1 + (K + 4) u23 mag1                                          S.elem_bound's accumulation term
    act none/ReLU:   pre = e_p (Lipschitz 1)
    act GELU:        pre = L e_p + n_ops u23 (|gelu(p)| + L e_p)                    L = sup |gelu'| computed in float64 by
                                                                                    `gelu_lipschitz`, n_ops = S.act_n_ops at |p| + e_p
    e_h            = pre + half_ulp_bf16(|h| + pre)                                 the bf16 pack of the hidden value (or the store)
    fc2:             E2 = e_h |W2|^T,   mag2 = (|h| + e_h) |W2|^T + |b2| + |res|,   e_2 = E2 + (H + 5) u23 mag2   (H + 4, and one more
                                                                                    rounding for the residual)
    bound          = e_2 + half_ulp_out(|ref| + e_2)
No factor is chosen by eye: every term is a counted rounding or a float64 propagation of one.  N.judge applies S.check_bound to every
element and S.check_bias where the project's condition holds (bf16 output, >= 4096 reference elements of |ref| >= 2^-6).

Routing gates restated here and checked on the CPU (tests/test_strict_lngemm_host.py): mv_ln_linear needs M >= 8192, mv_ln_mlp
M >= 1024, mv_ln_mlp_stream M >= 128.  Rows below a gate never reach these kernels; the GPU module asserts that the entry refuses
them (no silent fall-back) and places the tail shapes directly above the gate: M = gate (whole tiles), gate + 1, + 31 and + 33 (the
last tile holds 1, 31 and 1 rows past a tile edge), and 32 t + 5.

Worst |err| / bound of the honest emulations on the CPU (tests/test_strict_lngemm_host.py prints them with -s), at the smallest
ragged case of each kernel; the exact instrument is bit-equal at every one of them:
    ln_linear K = 96 0.482 (fp32 stream)   K = 192 0.389 (bf16 stream)
    ln_mlp96 0.025 (fp32 stream)   0.420 (bf16 stream)   0.025 / 0.022 (res, fp32 / bf16 in)
    ln_mlp_stream C = 192 0.011   C = 384 0.005          (fp32 outputs: the bound is made of the half ulps of the two bf16 packs
                                                          summed in absolute value over 96 .. 1536 terms; the errors add like a random walk)
Seeded defects (DEFECTS) and the instrument that rejects them in the emulation (E exact, B per-element bound, b rounding bias); `cmp`
marks those the former `_cmp(got, ref, 1e-2)` lets through on the same Gaussian data:
    neighbour_stats  E B         everywhere
    c_minus_1        E           at C = 96 and 192 (+-1 becomes 0.9961 in bf16), also B b at ln_linear K = 96         cmp: every kernel
                                 at C = 384 sqrt(383 / 384) leaves +-1 where it is: the streamed kernels also run the exact chain on
                                 MIDPOINT rows (instrument 1b below), which the C - 1 variance moves by one bf16 ulp: E at 192 and 384
    no_eps           B           the constant row (0 * rsqrt(0) or a residue times rsqrt of a residue); E cannot see it
    drop_wbeta       E, B at ln_linear                                                                                cmp: ln_mlp*, own residual
    drop_chunk       E, B but at C = 384                                                                              cmp: ln_mlp_stream C = 384
    swap_hidden      E, B at C = 96                                                                                   cmp: ln_mlp*, own residual
    res_prev_row     E B
    trunc_pack       E where eps shows (a_r = 1/4 rows), b where the output is bf16                                   cmp: every kernel
At the ln_mlp* kernels the per-element regime alone protects little: its bound sums the half ulps of two bf16 packs in absolute value
(honest ratios 0.005 .. 0.03), so drop_wbeta, swap_hidden (C >= 192) and drop_chunk (C = 384) pass it; the exact instruments are what
reject them.
Kernels whose LayerNorm FOLLOWS the accumulation get `post_ln_bound`: the accumulation's elem_bound pushed through the LayerNorm's
sensitivity, plus ln_ref_bound.  mv_cnblock_dw_fwd: cnb_exact (normalize = 0 in integers), cnb_sign (normalize = 1, outputs of exactly
+-1) and cnb_gauss (normalize = 1, bound and bias; emulation 0.986, MI355X 0.986: the bf16 store's half ulp is nearly all of the
bound).  mv_patch4_ln_fwd: patch4_gauss (emulation 0.005, MI355X 0.006).
mv_linear_lnout_fwd -> mv_linear_lnin_fwd: check_lnout (hi a correct rounding, |lo|, hi + lo, Chan mean and variance, every element
and row) and lnin_ref_bound (its docstring states the model); emulation 0.417 / 0.276, MI355X 0.417 / 0.276 at the two cases.
mv_se_scale_fwd and the activations fused into the conv / GEMM epilogues have the two instruments in tests/_strict.py ("fused
activations": S.through_act is the GELU line above for every activation, with this module's gelu_lipschitz) and run in
tests/test_strict_act_gpu.py.
"""
from __future__ import annotations

import functools

import numpy as np

from tests import _strict as S
from tests import _strict_norm as N
from tests._strict import bf, rng_of, half_ulp_out, check_exact  # noqa: F401

F32, F64 = np.float32, np.float64
EPS = 1e-5
U23 = 2.0 ** -23
SENTINEL = S.SENTINEL
LINEAR_MIN_M, MLP_MIN_M, STREAM_MIN_M = 8192, 1024, 128        # the _supported gates (stream1x1.hip, ln_mlp.hip, ln_mlp_stream.hip)


# ================================================================================================ case tables
def linear_grid(M, K, N_):
    """stream_go's arithmetic for the LN mode (TN = 4, 8 waves): (gx, gy, npass, waves in x, row tiles)."""
    wpitch = K * 2 + 16
    slab, patches = 128 * wpitch + 2 * 128 * 4, 8 * 32 * (64 * 4 + 16)
    tiles_n = -(-N_ // 128)
    npass = max(1, min((160 * 1024 - 1024 - patches) // slab, tiles_n))
    gy = -(-tiles_n // npass)
    tiles_m = -(-M // 32)
    gx = min(max(256 // gy, 1), -(-tiles_m // 8))
    return gx, gy, npass, gx * 8, tiles_m


def mlp_grid(M, waves=12):
    """ln_mlp_go: (blocks, tile stride of a wave, tiles)."""
    tiles = -(-M // 32)
    grid = min(-(-tiles // waves), 256)
    return grid, grid * waves, tiles


# M: the gate, one row / 31 / 33 rows in the last tile, and the smallest 32 t + 5 at which a wave walks to a second tile
LINEAR_M2 = 32 * 2048 + 5          # 8 waves x 256 blocks = 2048 tiles in flight: tile 2048 is wave 0's second and the ragged one
MLP_M2 = 32 * 3072 + 5             # 12 waves x 256 blocks
MLP_M2_W8 = 32 * 2048 + 5          # flag ln_mlp_waves=8: the kernel's PREFETCH path
LINEAR_CASES = [                   # (M, K, N, stream, flags)
    (8192 + 5, 96, 256, "fp32", ()), (8192 + 5, 96, 200, "bf16", ()), (8192 + 33, 96, 200, "fp32", ()),
    (LINEAR_M2, 96, 200, "fp32", ()),
    (8192 + 5, 192, 256, "bf16", ("ln_stream_192",)), (8192 + 1, 192, 200, "fp32", ("ln_stream_192",)),
]
MLP96_CASES = [(M, st, res, ()) for M in (1024, 1025, 1055, 1057) for st in ("fp32", "bf16") for res in (False, True)]
MLP96_SMALL = list(MLP96_CASES)
MLP96_CASES += [(MLP_M2, "fp32", False, ()), (MLP_M2, "bf16", True, ()), (MLP_M2_W8, "fp32", False, ("ln_mlp_waves=8",))]
# the per-element bound runs at the small shapes and at ONE second-tile shape (the float64 reference of 98 309 rows takes seconds); the
# bf16 / res second-tile shape and the ln_mlp_waves=8 path have the exact test only
MLP96_BOUND_CASES = MLP96_SMALL + [(MLP_M2, "fp32", False, ())]
STREAM_CASES = [(M, C, res) for C, Ms in ((192, (128, 133, 261)), (384, (128, 133, 197))) for M in Ms for res in (False, True)]


def linear_id(c):
    return f"M{c[0]}_K{c[1]}_N{c[2]}_{c[3]}"


def mlp96_id(c):
    return f"M{c[0]}_{c[1]}" + ("_res" if c[2] else "") + ("_" + c[3][0].replace("=", "") if c[3] else "")


def stream_id(c):
    return f"C{c[1]}_M{c[0]}" + ("_res" if c[2] else "")


def linear_kernel(K, stream):
    return f"stream1x1_ln_{'f32in' if stream == 'fp32' else 'bf16in'}_k{K}"


def mlp96_kernel(stream, res):
    if res:
        return "ln_mlp96_res_f32in" if stream == "fp32" else "ln_mlp96_res_bf16in"
    return "ln_mlp96_f32stream" if stream == "fp32" else "ln_mlp96_bf16stream"


def stream_kernel(C, res):
    return f"ln_mlp_stream_c{C}_" + ("res" if res else "f32stream")


def stream_fragments(w1f, w2):
    """The fragment order of mv_ln_mlp_stream_fwd (include/eqxvision_amd.h): w1f [Hd][C], w2 [C][Hd] -> (w1 stream, w2 stream)."""
    Hd, C = w1f.shape
    a = w1f.reshape(Hd // 256, 8, 32, C // 16, 2, 8).transpose(0, 1, 3, 4, 2, 5)
    b = w2.reshape(C // 32, 32, Hd // 256, 16, 2, 8).transpose(2, 0, 3, 4, 1, 5)
    return np.ascontiguousarray(a), np.ascontiguousarray(b)


# ================================================================================================ instrument 1: +-1 rows
def pm1_rows_x(M, C, stream, seed, mult16=False):
    """(x (M, C) float32, signs (M, C), a (M,), m (M,)): x = m_r + a_r * sign.  mult16: a_r in {16, 64} and |m_r| <= 4 a_r (the bf16
    residual stream of ln_mlp: x + an integer multiple of 16 stays a bf16 value); else a_r cycles through 1/4, 1, 4, 16."""
    rng = rng_of(seed)
    cyc, jmax = ((16.0, 64.0), 4) if mult16 else ((0.25, 1.0, 4.0, 16.0), 8)
    a = np.array(cyc)[np.arange(M) % len(cyc)]
    m = rng.integers(-jmax, jmax + 1, M) * a
    sg = rng.permuted(np.tile(np.repeat(np.array([1, -1], np.int8), C // 2), (M, 1)), axis=1)
    x = (m[:, None] + a[:, None] * sg).astype(F32)
    if stream == "bf16":
        assert np.array_equal(bf(x), x), "+-1 rows: an entry is not a bf16 value"
    return x, sg.astype(F32), a, m


def prove_pm1(name, x, sg, a, m, eps=EPS):
    """The construction's preconditions, asserted in float64 before a launch (module docstring)."""
    M, C = x.shape
    assert C % 2 == 0 and (sg.sum(1) == 0).all() and (np.abs(sg) == 1).all(), f"{name}: signs are not balanced"
    assert (np.frexp(a)[0] == 0.5).all() and (a >= 0.25).all(), f"{name}: a_r is not a power of two >= 1/4"
    assert (np.abs(m) <= 64 * a).all() and np.array_equal(x.astype(F64), m[:, None] + a[:, None] * sg), name
    r = np.arange(M)
    for nb in (np.minimum(r ^ 1, M - 1), np.maximum(r - 1, 0), np.minimum(r + 1, M - 1)):
        other = nb != r
        ratio = a[nb] / a
        assert ((ratio >= 4) | (ratio <= 0.25))[other].all(), f"{name}: neighbouring rows are closer than a factor 4 in a_r"
        assert (sg[nb] != sg).any(1)[other].all(), f"{name}: neighbouring rows share a sign pattern"
    worst_dev = worst_all = 0.0
    for r0 in range(0, M, 8192):                                  # slabs: the largest case has 98 309 rows
        n, bound = N.ln_ref_bound(x[r0:r0 + 8192], None, None, None, eps, "fp32")
        assert np.array_equal(np.sign(n), sg[r0:r0 + 8192]), name
        dev = np.abs(np.abs(n) - 1.0)
        worst_dev, worst_all = max(worst_dev, float(dev.max())), max(worst_all, float((dev + bound).max()))
    assert worst_dev < 2.0 ** -10, f"{name}: a / sqrt(a^2 + eps) is {worst_dev} from 1"
    assert worst_all < 2.0 ** -9, f"{name}: the fp32 error bound leaves the bf16 rounding interval of 1 ({worst_all})"
    return worst_dev, worst_all


def _distinct(w):
    w = np.asarray(w)
    return len({r.tobytes() for r in w}) == w.shape[0] and len({c.tobytes() for c in np.ascontiguousarray(w.T)}) == w.shape[1]


def _ternary(rng, rows, kred, nnz):
    p = nnz / kred
    return rng.choice(np.array([-1.0, 0.0, 1.0], F32), (rows, kred), p=[p / 2, 1 - p, p / 2])


@functools.lru_cache(maxsize=None)
def linear_exact(M, K, N_, stream, act, seed=100):
    """x (+-1 rows), W' = W diag(gamma) (W in {-1, 0, 1}, gamma in {1, 2} per k), b' = b + W beta (integers), the integer
    reference.  Returns (x, W', b', b (without the W beta term), ref)."""
    name = f"ln_linear/exact/{M}x{K}x{N_}/{stream}/act{act}"
    x, sg, a, m = pm1_rows_x(M, K, stream, seed + K)
    prove_pm1(name, x, sg, a, m)
    rng = rng_of(seed + 1 + K + N_)
    W = _ternary(rng, N_, K, 32)
    gamma, beta = rng.choice(np.array([1.0, 2.0], F32), K), S.int_tensor(rng, (K,), 2)
    b = S.int_tensor(rng, (N_,), 8)
    wf = bf(W * gamma[None, :])
    assert np.array_equal(wf, W * gamma[None, :]) and _distinct(wf), f"{name}: weight patterns repeat"
    bfold = (b + W @ beta).astype(F32)
    ref, mag = S.gemm_ref(sg, wf, None, bfold, None, act)
    S.prove_exact(name, ref, mag, [wf], stored=[wf], out="bf16")
    for v in (x, wf, bfold, ref):
        v.setflags(write=False)
    return x, wf, bfold, b, ref


def gelu_exact_from():
    """The smallest |x| (to 2^-10) at which |t| > 128 in gelu_tanh_f's own float32 arithmetic, by bisection on a monotone |t|."""
    def t_of(x):
        x = F32(x)
        return abs(float(x * F32(float(S._GELU_K1) * float(x * x) + float(S._GELU_K0))))
    lo, hi = 1.0, 32.0
    assert t_of(lo) < 128 < t_of(hi)
    while hi - lo > 2.0 ** -10:
        mid = 0.5 * (lo + hi)
        lo, hi = (lo, mid) if t_of(mid) > 128 else (mid, hi)
    return hi


@functools.lru_cache(maxsize=None)
def mlp_exact(M, C, stream, with_res, seed=200):
    """The exact LN -> fc1 -> GELU -> fc2 -> + residual chain.  Returns (x, res or None, W1', b1', b1, W2, b2, ref, out dtype)."""
    Hd = 4 * C
    out = "fp32" if with_res else stream
    name = f"ln_mlp/exact/{M}x{C}/{stream}/res{int(with_res)}"
    x, sg, a, m = pm1_rows_x(M, C, stream, seed + C, mult16=out == "bf16")
    prove_pm1(name, x, sg, a, m)
    rng = rng_of(seed + 1 + C)
    W1 = 16.0 * _ternary(rng, Hd, C, 16)
    gamma, beta = rng.choice(np.array([1.0, 2.0], F32), C), S.int_tensor(rng, (C,), 2)
    b1 = 16.0 * S.int_tensor(rng, (Hd,), 4)
    w1f = bf(W1 * gamma[None, :])
    assert np.array_equal(w1f, W1 * gamma[None, :]) and _distinct(w1f), name
    b1f = (b1 + W1 @ beta).astype(F32)
    W2 = np.zeros((C, Hd), F32)                                   # four +-1 per hidden unit: about 16 per output channel
    for u in range(Hd):
        W2[rng.choice(C, 4, replace=False), u] = rng.choice(np.array([-1.0, 1.0], F32), 4)
    assert _distinct(W2), f"{name}: fc2 weight patterns repeat"
    b2 = S.int_tensor(rng, (C,), 8) * (16.0 if out == "bf16" else 1.0)
    res = S.int_tensor(rng, (M, C), 64) if with_res else None
    # every pre-activation is a multiple of 16 at or beyond the point where GELU is an exact ReLU
    assert gelu_exact_from() <= 16.0
    p, mag1 = S.gemm_ref(sg, w1f, None, b1f, None, 0)
    assert np.array_equal(np.ldexp(p, -4), np.rint(np.ldexp(p, -4)))
    h = np.maximum(p, 0.0)
    S.prove_exact(name + "/fc1", h, mag1, [w1f], stored=[w1f], out="bf16", frac_bits=-4)
    r = x.astype(F64) if res is None else res.astype(F64)
    ref = r + h @ W2.astype(F64).T + b2
    mag2 = h @ np.abs(W2).astype(F64).T + np.abs(b2) + np.abs(r)
    if out == "bf16":
        S.prove_exact(name + "/fc2", ref, mag2, [W2], hidden=[h], out="bf16", frac_bits=-4)
    else:                                                          # x holds quarters: integers after two more bits
        S.prove_exact(name + "/fc2", ref, mag2, [W2], hidden=[h], out="fp32", frac_bits=2, hidden_max=4 * 4096)
    for v in (x, w1f, b1f, W2, b2, ref) + (() if res is None else (res,)):
        v.setflags(write=False)
    return x, res, w1f, b1f, b1, W2, b2, ref, out


# ================================================================================================ instrument 2: data, reference, bound
def gauss_rows(M, C, stream, seed):
    """ln_linear_case's rows (per-row scale in [0.5, 2], offset in [-1, 1]); every seventh row carries a common offset of 50 of its
    standard deviations; row 5 is constant (0.3)."""
    rng = rng_of(seed)
    sc = rng.uniform(0.5, 2.0, (M, 1))
    x = rng.standard_normal((M, C)) * sc + rng.uniform(-1.0, 1.0, (M, 1))
    x[3::7] += 50.0 * sc[3::7] * np.where(np.arange(len(sc[3::7])) % 2 == 0, 1.0, -1.0)[:, None]
    x[5] = 0.3
    return S.q_of(stream)(x.astype(F32))


@functools.lru_cache(maxsize=None)
def gelu_lipschitz():
    """sup |gelu_tanh'| in float64: the analytic derivative on a grid of step h = 2^-12 over [-12, 12], plus h / 2 max |gelu''| for
    what lies between two grid points; beyond +-12 the derivative is within 1e-12 of its limits 0 and 1."""
    h = 2.0 ** -12
    x = np.arange(-12.0, 12.0 + h, h)
    c = np.sqrt(2.0 / np.pi)
    s = 1.0 / (1.0 + np.exp(-2.0 * c * (x + 0.044715 * x ** 3)))
    g1 = s + x * s * (1.0 - s) * 2.0 * c * (1.0 + 3.0 * 0.044715 * x * x)
    assert abs(g1[0]) < 1e-12 and abs(g1[-1] - 1.0) < 1e-12
    g2 = np.abs(np.diff(g1)).max() / h
    return float(np.abs(g1).max() + 0.5 * h * g2)


def _through_act(p, e_p, act, out):
    """(ref, bound) of out(act(p)) for a pre-activation known to e_p (module docstring)."""
    if act in (0, 1):
        ref, pre = (p if act == 0 else np.maximum(p, 0.0)), e_p
    else:
        L = gelu_lipschitz()
        ref = S.act64(p, "gelu_tanh")
        pre = L * e_p + S.act_n_ops(np.abs(p) + e_p, "gelu_tanh") * U23 * (np.abs(ref) + L * e_p)
    return ref, pre + half_ulp_out(np.abs(ref) + pre, out)


def _fc1(x, wf, bfold, eps):
    n, e_ln = N.ln_ref_bound(x, None, None, None, eps, "bf16")
    aw = np.abs(wf).astype(F64)
    p = n @ wf.astype(F64).T + bfold.astype(F64)
    mag = (np.abs(n) + e_ln) @ aw.T + np.abs(bfold).astype(F64)
    return p, e_ln @ aw.T + (x.shape[1] + 4) * U23 * mag


def linear_ref_bound(x, wf, bfold, act, eps=EPS, out="bf16"):
    ref, bound = [], []
    for r0 in range(0, x.shape[0], 8192):
        p, e_p = _fc1(x[r0:r0 + 8192], wf, bfold, eps)
        r, b = _through_act(p, e_p, act, out)
        ref.append(r), bound.append(b)
    return np.concatenate(ref), np.concatenate(bound)


def mlp_ref_bound(x, res, w1f, b1f, w2, b2, out, eps=EPS):
    Hd = w1f.shape[0]
    w2_64, aw2 = w2.astype(F64), np.abs(w2).astype(F64)
    ref, bound = [], []
    for r0 in range(0, x.shape[0], 8192):
        xs = x[r0:r0 + 8192]
        p, e_p = _fc1(xs, w1f, b1f, eps)
        h, e_h = _through_act(p, e_p, 2, "bf16")
        r = (xs if res is None else res[r0:r0 + 8192]).astype(F64)
        y = r + h @ w2_64.T + b2.astype(F64)
        mag2 = (np.abs(h) + e_h) @ aw2.T + np.abs(b2).astype(F64) + np.abs(r)
        e2 = e_h @ aw2.T + (Hd + 5) * U23 * mag2
        ref.append(y), bound.append(e2 + half_ulp_out(np.abs(y) + e2, out))
    return np.concatenate(ref), np.concatenate(bound)


@functools.lru_cache(maxsize=None)
def linear_gauss(M, K, N_, stream, act, seed=300):
    """(x, W' bf16-rounded, b', b, ref, bound): Gaussian operands as _cases.ln_linear_case draws them."""
    x = gauss_rows(M, K, stream, seed + K)
    rng = rng_of(seed + 1 + K + N_)
    g, be = rng.uniform(0.5, 1.5, K).astype(F32), (0.1 * rng.standard_normal(K)).astype(F32)
    w, b = (rng.standard_normal((N_, K)) / np.sqrt(K)).astype(F32), (0.1 * rng.standard_normal(N_)).astype(F32)
    wf, bfold = bf(w * g[None, :]), (b + w @ be).astype(F32)
    ref, bound = linear_ref_bound(x, wf, bfold, act)
    for v in (x, wf, bfold, ref, bound):
        v.setflags(write=False)
    return x, wf, bfold, b, ref, bound


@functools.lru_cache(maxsize=None)
def mlp_gauss(M, C, stream, with_res, seed=400):
    """(x, res or None, W1', b1', b1, W2 bf16-rounded, b2, ref, bound, out dtype): operands as _cases.ln_mlp_case draws them."""
    Hd = 4 * C
    out = "fp32" if with_res else stream
    x = gauss_rows(M, C, stream, seed + C)
    rng = rng_of(seed + 1 + C)
    g, be = rng.uniform(0.5, 1.5, C).astype(F32), (0.1 * rng.standard_normal(C)).astype(F32)
    w1, b1 = (rng.standard_normal((Hd, C)) / np.sqrt(C)).astype(F32), (0.1 * rng.standard_normal(Hd)).astype(F32)
    w2, b2 = bf(rng.standard_normal((C, Hd)) / np.sqrt(Hd)), (0.1 * rng.standard_normal(C)).astype(F32)
    res = rng.standard_normal((M, C)).astype(F32) if with_res else None
    w1f, b1f = bf(w1 * g[None, :]), (b1 + w1 @ be).astype(F32)
    ref, bound = mlp_ref_bound(x, res, w1f, b1f, w2, b2, out)
    for v in (x, w1f, b1f, w2, b2, ref, bound) + (() if res is None else (res,)):
        v.setflags(write=False)
    return x, res, w1f, b1f, b1, w2, b2, ref, bound, out


def cmp_1e2(got, ref):
    """The former check, restated: tests/_cases.py `_cmp(got, ref, 1e-2)`."""
    got, ref = np.asarray(got, F64), np.asarray(ref, F64)
    return bool(np.isfinite(got).all() and np.abs(got - ref).max() <= 1e-2 * max(1.0, np.abs(ref).max()))


# ================================================================================================ emulations
DEFECTS = ("neighbour_stats", "c_minus_1", "no_eps", "drop_wbeta", "drop_chunk", "swap_hidden", "res_prev_row", "trunc_pack")
LINEAR_DEFECTS = tuple(d for d in DEFECTS if d not in ("swap_hidden", "res_prev_row"))
SWAP_UNITS = (4, 8)               # a pair the LDS permutation of W2 puts next to each other (ln_mlp.hip: hidden {+0..3, +8..11} per slot)


def _finish_stats(qsum, C, eps, defect):
    inv = F32(1) / F32(C)
    var = qsum * (F32(1) / F32(C - 1) if defect == "c_minus_1" else inv)
    return N._rsqrt32(var if defect == "no_eps" else var + F32(eps))


def _normalise(x, eps, kind, defect):
    """The bf16 fragment values n = pack((x - mean) * rstd) in float32, in the kernel's order.  kind "half": stream1x1's LN mode and
    ln_mlp96 -- lane half fh holds elements 16 kk + 8 fh + e, adds them in (kk, e) order, then the other half's sum; the squares by
    fmaf.  kind "stream": ln_mlp_stream -- C / 12 lanes per row with three float4 each, pairwise sums, an xor butterfly."""
    x = np.asarray(x, F32)
    M, C = x.shape
    inv = F32(1) / F32(C)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        if kind == "half":
            v = x.reshape(M, C // 16, 2, 8)
            s = np.zeros((M, 2), F32)
            for kk in range(C // 16):
                for e in range(8):
                    s = s + v[:, kk, :, e]
            mean = (s[:, 0] + s[:, 1]) * inv
            d = v - mean[:, None, None, None]
            q = np.zeros((M, 2), F32)
            for kk in range(C // 16):
                for e in range(8):
                    dd = d[:, kk, :, e].astype(F64)
                    q = (dd * dd + q.astype(F64)).astype(F32)
            rstd = _finish_stats(q[:, 0] + q[:, 1], C, eps, defect)
        else:
            lpr = C // 12
            v = x.reshape(M, 3, lpr, 4)
            s = np.zeros((M, lpr), F32)
            for i in range(3):
                s = s + ((v[:, i, :, 0] + v[:, i, :, 1]) + (v[:, i, :, 2] + v[:, i, :, 3]))
            mean = N._butterfly(s, lpr) * inv
            d = v - mean[:, None, None, None]
            q = np.zeros((M, lpr), F32)
            for i in range(3):
                sq = d[:, i] * d[:, i]
                q = q + ((sq[..., 0] + sq[..., 1]) + (sq[..., 2] + sq[..., 3]))
            rstd = _finish_stats(N._butterfly(q, lpr), C, eps, defect)
        if defect == "neighbour_stats":
            src = np.arange(M) ^ 1
            src = np.where(src < M, src, np.arange(M))
            mean, rstd = mean[src], rstd[src]
        n = (x - mean[:, None]) * rstd[:, None]
    return S.store(n, "bf16", "trunc" if defect == "trunc_pack" else "rne")


def _gemm32(a, w, drop_chunk=None, acc=None):
    """fp32 accumulation of a . w^T in 16-wide k-steps (one MFMA each), starting from `acc`."""
    a, w = np.asarray(a, F32), np.asarray(w, F32)
    acc = np.zeros((a.shape[0], w.shape[0]), F32) if acc is None else np.array(acc, F32)
    with np.errstate(invalid="ignore", over="ignore"):
        for c, k0 in enumerate(range(0, a.shape[1], 16)):
            if c != drop_chunk:
                acc = acc + a[:, k0:k0 + 16] @ w[:, k0:k0 + 16].T
    return acc


def emu_ln_linear(x, wf, bfold, b, act, eps=EPS, defect=None):
    """stream1x1_kernel<LN>: the fragment, the MFMAs, fmaf(acc, 1, shift), the activation, the bf16 store.  Defects (one at a time):
    neighbour_stats (statistics of row m ^ 1), c_minus_1, no_eps, drop_wbeta (columns >= 128 get b, not b + W beta), drop_chunk (k-step
    2 is not accumulated), trunc_pack (truncation at the fragment pack and the store)."""
    n = _normalise(x, eps, "half", defect)
    sh = np.array(bfold, F32)
    if defect == "drop_wbeta":
        sh[128:] = np.asarray(b, F32)[128:]
    with np.errstate(invalid="ignore", over="ignore"):
        y = _gemm32(n, wf, 2 if defect == "drop_chunk" else None) + sh
        y = S.act32(y, {0: "none", 1: "relu", 2: "gelu_tanh"}[act])
    return S.store(y, "bf16", "trunc" if defect == "trunc_pack" else "rne")


def emu_ln_mlp(x, res, w1f, b1f, b1, w2, b2, out, kind, eps=EPS, defect=None):
    """ln_mlp96_kernel (kind "half": 32-row tiles, the fc2 accumulators START as the residual, + b2 last) and ln_mlp_stream*_kernel
    (kind "stream": C = 192 -> 128-row tiles, 384 -> 64; (acc + b2) + residual).  Defects as emu_ln_linear's (drop_wbeta: hidden units
    >= 128), and swap_hidden (hidden units SWAP_UNITS trade places in W2), res_prev_row (the rows of the last, ragged tile take the
    residual of row m - 1)."""
    x = np.asarray(x, F32)
    M, C = x.shape
    mode = "trunc" if defect == "trunc_pack" else "rne"
    n = _normalise(x, eps, kind, defect)
    sh = np.array(b1f, F32)
    if defect == "drop_wbeta":
        sh[128:] = np.asarray(b1, F32)[128:]
    with np.errstate(invalid="ignore", over="ignore"):
        p = _gemm32(n, w1f, 2 if defect == "drop_chunk" else None) + sh
        h = S.store(S.act32(p, "gelu_tanh"), "bf16", mode)
    w2e = np.array(w2, F32)
    if defect == "swap_hidden":
        w2e[:, list(SWAP_UNITS)] = w2e[:, list(SWAP_UNITS)[::-1]]
    r = np.array(x if res is None else res, F32)
    if defect == "res_prev_row":
        tile = 32 if kind == "half" else (128 if C == 192 else 64)
        r0 = (M // tile) * tile if M % tile else M - tile
        r[r0:] = r[r0 - 1:M - 1].copy()
    with np.errstate(invalid="ignore", over="ignore"):
        if kind == "half":
            y = _gemm32(h, w2e, acc=r) + np.asarray(b2, F32)
        else:
            y = (_gemm32(h, w2e) + np.asarray(b2, F32)) + r
    return S.store(y, out, mode)


# ================================================================================================ mv_cnblock_dw_fwd: the two exact cases
CNB_CASES = [(96, "fp32"), (96, "bf16"), (192, "fp32"), (192, "bf16")]           # (C, x dtype): TW = 32 and 16


def cnb_tile(C):
    """cnblock.hip's cnb_tile: output pixels of one row per workgroup."""
    tw = 32
    while tw > 4 and tw * C > 4096:
        tw >>= 1
    return tw


def cnb_shape(C):
    """(N, H, W): two images, nine rows (every vertical padding case of the 7 x 7 window), a width of TW + 5 (a ragged second tile)."""
    return 2, 9, cnb_tile(C) + 5


@functools.lru_cache(maxsize=None)
def cnb_exact(C):
    """normalize = 0 in integers: x in [-2, 2], filters in +-1, +-2 (a depthwise filter has one channel: no zero tap) with a pattern of their own per tap and per channel, integer bias;
    |d| <= 49 * 4 + 8 is exact in fp32 and bf16.  Returns (x NHWC, w [7][7][C], bias, ref)."""
    rng = rng_of(500 + C)
    N_, H, W = cnb_shape(C)
    x, w, bias = S.int_tensor(rng, (N_, H, W, C), 2), S.int_nz(rng, (7, 7, C), 2), S.int_tensor(rng, (C,), 8)
    assert _distinct(w.reshape(49, C)), "cnblock/exact: two taps or two channels share a filter pattern"
    wk = np.ascontiguousarray(w.transpose(2, 0, 1))[..., None]                   # [K = C][7][7][1]
    ref, mag = S.conv_ref(x, wk, None, bias, None, 0, 1, 3, 1, C)
    S.prove_exact(f"cnblock/exact/C{C}", ref, mag, [wk[i:i + 1] for i in range(C)], stored=[x, w], out="bf16")
    for v in (x, w, bias, ref):
        v.setflags(write=False)
    return x, w, bias, ref


@functools.lru_cache(maxsize=None)
def cnb_sign(C):
    """normalize = 1 with an exact answer: x constant over the channels (integers in [-2, 2]), w[r][s][c] = sigma_c f[r][s] with
    balanced signs sigma and f a permutation of 1 .. 49, no bias.  Then d[p][c] = sigma_c v_p with the integer v = f * x: the channel
    mean is 0 in any order of summation, the variance v^2, and the normalised value sigma_c v / sqrt(v^2 + eps) is within 2^-10 of
    +-1 for every integer v != 0 -- asserted here together with the fp32 error ln_ref_bound allows, as in prove_pm1.  Returns
    (x, w, ref, keep): `keep` marks the pixels with v != 0; the others are skipped."""
    rng = rng_of(600 + C)
    N_, H, W = cnb_shape(C)
    xi = S.int_tensor(rng, (N_, H, W, 1), 2)
    x = np.ascontiguousarray(np.broadcast_to(xi, (N_, H, W, C)))
    f = rng.permutation(np.arange(1.0, 50.0)).reshape(7, 7).astype(F32)
    sigma = rng.permuted(np.repeat(np.array([1.0, -1.0], F32), C // 2))
    w = np.ascontiguousarray(f[:, :, None] * sigma[None, None, :])
    v = S._conv64(xi, f[None, :, :, None], 1, 3, 1, 1)[..., 0]                    # (N, H, W) integers, |v| <= 2450
    assert np.array_equal(v, np.rint(v)) and np.abs(v).max() * C < S.ACC_INT_MAX
    d = v[..., None] * sigma.astype(F64)
    keep = v != 0
    assert keep.mean() > 0.9
    n, bound = N.ln_ref_bound(d[keep], None, None, None, EPS, "fp32")
    assert float((np.abs(np.abs(n) - 1.0)).max()) < 2.0 ** -10 and float((np.abs(np.abs(n) - 1.0) + bound).max()) < 2.0 ** -9
    ref = np.sign(d)
    for a in (x, w, ref, keep):
        a.setflags(write=False)
    return x, w, ref, keep


def emu_cnblock(x, w, bias, normalize, out, eps=EPS, defect=None):
    """cnblock_dw_kernel in float32: fmaf over the taps in (r, s) order, + bias, and for normalize = 1 the statistics as one wave
    takes them (lane l adds channels l, l + 64, ...; xor butterfly; two passes), (d - mean) * rstd.  Defects: neighbour_stats (the
    statistics of pixel w ^ 1 of the same row), c_minus_1, no_eps, trunc_pack, and drop_tap (tap (6, 6) is not accumulated)."""
    x = np.asarray(x, F32)
    N_, H, W, C = x.shape
    xp = np.zeros((N_, H + 6, W + 6, C), F32)
    xp[:, 3:3 + H, 3:3 + W] = x
    acc = np.zeros((N_, H, W, C), F64)
    for r in range(7):
        for s in range(7):
            if defect == "drop_tap" and (r, s) == (6, 6):
                continue
            acc = (xp[:, r:r + H, s:s + W].astype(F64) * np.asarray(w, F32)[r, s].astype(F64) + acc).astype(F32).astype(F64)
    d = acc.astype(F32)
    if bias is not None:
        d = d + np.asarray(bias, F32)
    mode = "trunc" if defect == "trunc_pack" else "rne"
    if not normalize:
        return S.store(d, out, mode)
    rows = d.reshape(-1, C)
    lanes = np.zeros((rows.shape[0], 64), F32)
    for c0 in range(0, C, 64):
        blk = rows[:, c0:c0 + 64]
        lanes[:, :blk.shape[1]] = lanes[:, :blk.shape[1]] + blk
    mean = N._butterfly(lanes, 64) * (F32(1) / F32(C))
    q = np.zeros((rows.shape[0], 64), F32)
    for c0 in range(0, C, 64):
        dv = (rows[:, c0:c0 + 64] - mean[:, None]).astype(F64)
        q[:, :dv.shape[1]] = (dv * dv + q[:, :dv.shape[1]].astype(F64)).astype(F32)
    rstd = _finish_stats(N._butterfly(q, 64), C, eps, defect)
    if defect == "neighbour_stats":
        wi = np.arange(rows.shape[0]) % W
        src = np.arange(rows.shape[0]) + np.where((wi ^ 1) < W, (wi ^ 1) - wi, 0)
        mean, rstd = mean[src], rstd[src]
    with np.errstate(invalid="ignore", over="ignore"):
        y = (rows - mean[:, None]) * rstd[:, None]
    return S.store(y, out, mode).reshape(N_, H, W, C)


# ================================================================================================ instrument 1b: midpoint rows
# The +-1 rows cannot see a variance divided by C - 1 once C is large: sqrt(383 / 384) = 0.9987 leaves 1.0 where it is in bf16.  These
# rows can.  k entries are m + a (C - k), the other C - k are m - a k: the mean is m, the variance a^2 k (C - k), and the normalised
# values are +sqrt((C - k) / k) and -sqrt(k / (C - k)) (times 1 - O(eps / a^2)).  k is CHOSEN so that one of the two lies just above the
# midpoint of two bf16 values -- by less than the factor sqrt((C - 1) / C) takes away, by more than the fp32 error ln_ref_bound allows --
# and the other well clear of any midpoint.  The fragment is then a known bf16 value, and the C - 1 variance moves it one ulp down.
def _bf16_mid_margin(v):
    """(v - midpoint below v) / v for v > 0 where the midpoint is that of the two bf16 values around v; negative: v is in the lower half."""
    lo = S.bf16_truncate(np.asarray(v, F32)).astype(F64)
    return (np.asarray(v, F64) - (lo + half_ulp_out(lo, "bf16"))) / v


def midpoint_ks(C, n=4, clear=2.0 ** -12):
    """The first n counts k in [0.3 C, 0.7 C] with one normalised value in the window above a midpoint, the other `clear` (relative) from
    every midpoint and bf16 value's edge.  The window is (clear, eps_C - clear) with eps_C = 1 - sqrt((C - 1) / C)."""
    eps_c = 1.0 - np.sqrt((C - 1.0) / C)
    out = []
    for k in range(int(0.3 * C), int(0.7 * C) + 1):
        vp, vm = np.sqrt((C - k) / k), np.sqrt(k / (C - k))
        mp, mm = float(_bf16_mid_margin([vp])[0]), float(_bf16_mid_margin([vm])[0])
        hit_p, hit_m = clear < mp < eps_c - clear, clear < mm < eps_c - clear
        far_p, far_m = abs(mp) > eps_c + clear, abs(mm) > eps_c + clear
        if (hit_p and (far_m or hit_m)) or (hit_m and (far_p or hit_p)):
            out.append(k)
    assert len(out) >= n, f"C = {C}: only {len(out)} usable counts"
    return out[:n]


def midpoint_rows_x(M, C, seed):
    """(x, k per row, sign pattern): fp32 rows as described above, a_r cycling through 1/4, 1, 4 and m_r = j a_r, |j| <= 8."""
    rng = rng_of(seed)
    ks = np.array(midpoint_ks(C))[np.arange(M) % 4]
    a = np.array((0.25, 1.0, 4.0))[np.arange(M) % 3]
    m = rng.integers(-8, 9, M) * a
    plus = np.stack([rng.permutation(C) < k for k in ks])
    x = m[:, None] + a[:, None] * np.where(plus, (C - ks)[:, None], -ks[:, None])
    assert np.array_equal(x.astype(F32).astype(F64), x)
    return x.astype(F32), ks, plus


def prove_midpoint(name, x, eps=EPS):
    """The fragment of every element is ONE bf16 value over the whole interval ln_ref_bound allows the fp32 result (returned), and with
    the variance over C - 1 at least a quarter of the elements land on another one."""
    C = x.shape[1]
    n, bound = N.ln_ref_bound(x, None, None, None, eps, "fp32")
    frag = bf(n)
    assert np.array_equal(bf(n - bound), frag) and np.array_equal(bf(n + bound), frag), f"{name}: a value is too near a bf16 midpoint"
    nd = n * np.sqrt((C - 1.0) / C)
    moved = (bf(nd - bound) != frag) & (bf(nd + bound) != frag)
    assert moved.mean() > 0.25, f"{name}: the C - 1 variance moves only {moved.mean():.3f} of the fragment"
    return frag.astype(F64)


@functools.lru_cache(maxsize=None)
def mlp_midpoint(M, C, with_res, seed=700):
    """The exact chain on midpoint rows.  Every hidden unit reads ONE channel with a weight of +-16 or +-32 times gamma (gamma in {1, 2};
    beta = 0, b1 = 0): its pre-activation is a power of two times a bf16 value of magnitude >= 0.63 * 16 > gelu_exact_from(), so GELU is
    an exact ReLU and the hidden value a bf16 value.  fc2 in {-1, 0, 1}, integer b2 and residual: every sum is a multiple of 2^-4 below
    2^20.  Returns (x, res or None, W1', b1', W2, b2, ref)."""
    Hd = 4 * C
    name = f"ln_mlp/midpoint/{M}x{C}/res{int(with_res)}"
    x, ks, _ = midpoint_rows_x(M, C, seed + C)
    frag = prove_midpoint(name, x)
    rng = rng_of(seed + 1 + C)
    gamma = rng.choice(np.array([1.0, 2.0], F32), C)
    w1f = np.zeros((Hd, C), F32)
    unit = rng.permutation(Hd).reshape(C, 4)                      # the four hidden units of channel c
    for j, wv in enumerate((16.0, -16.0, 32.0, -32.0)):
        w1f[unit[:, j], np.arange(C)] = wv * gamma
    assert np.array_equal(bf(w1f), w1f) and _distinct(w1f)
    b1f = np.zeros(Hd, F32)
    W2 = np.zeros((C, Hd), F32)
    for u in range(Hd):
        W2[rng.choice(C, 4, replace=False), u] = rng.choice(np.array([-1.0, 1.0], F32), 4)
    assert _distinct(W2)
    b2 = S.int_tensor(rng, (C,), 8)
    res = S.int_tensor(rng, (M, C), 64) if with_res else None
    p = frag @ w1f.astype(F64).T
    assert float(np.abs(p).min()) >= gelu_exact_from()
    h = np.maximum(p, 0.0)
    assert np.array_equal(bf(h).astype(F64), h), f"{name}: a hidden value is not a bf16 value"
    r = x.astype(F64) if res is None else res.astype(F64)
    ref = r + h @ W2.astype(F64).T + b2
    mag2 = h @ np.abs(W2).astype(F64).T + np.abs(b2) + np.abs(r)
    S.prove_exact(name, ref, mag2, [w1f, W2], hidden=[h], out="fp32", frac_bits=4, hidden_max=1 << 20)
    assert float(mag2.max()) * 16 < 1 << 20
    for v in (x, w1f, b1f, W2, b2, ref) + (() if res is None else (res,)):
        v.setflags(write=False)
    return x, res, w1f, b1f, W2, b2, ref


# ================================================================================================ LayerNorm AFTER the accumulation
def post_ln_bound(d, e_d, eps, out, gamma=None, beta=None, k_mean=2, k_mul=3, k_add=2):
    """(ref, bound) of out((d - mean) / sqrt(var + eps) * gamma + beta) over the last axis when the kernel's d is within e_d (per
    element) of the float64 d.  Two parts, both from the float64 row statistics:
      sensitivity   n_i = (d_i - mu) / s.  A perturbation t (|t_j| <= e_j) moves mu by at most mean(e), s by (1 / C) sum n_j (t_j - dmu)
                    = (1 / C) sum n_j t_j (sum n_j = 0), i.e. by at most mean(|n| e); to first order
                    |dn_i| <= (e_i + mean(e)) / s + |n_i| mean(|n| e) / s.  The second-order remainder is below (C + 2) (max e / s)^2,
                    added whole.  Times |gamma_i|.
      arithmetic    _strict_norm.ln_ref_bound on d: the statistics, the normalisation and the affine in fp32, any order."""
    d, e = np.asarray(d, F64), np.asarray(e_d, F64)
    C = d.shape[-1]
    ref, b_ln = N.ln_ref_bound(d, gamma, beta, None, eps, "fp32", k_mean=k_mean, k_mul=k_mul, k_add=k_add)
    s = np.sqrt(d.var(-1, keepdims=True) + float(F32(eps)))
    n = (d - d.mean(-1, keepdims=True)) / s
    me, mne = e.mean(-1, keepdims=True), (np.abs(n) * e).mean(-1, keepdims=True)
    sens = (e + me) / s + np.abs(n) * mne / s + (C + 2) * (e.max(-1, keepdims=True) / s) ** 2
    pre = sens * (1.0 if gamma is None else np.abs(np.asarray(gamma, F64))) + b_ln
    return ref, pre + half_ulp_out(np.abs(ref) + pre, out)


@functools.lru_cache(maxsize=None)
def cnb_gauss(C, xdt):
    """(x, w bf16-rounded, bias, ref, bound) for normalize = 1: Gaussian map with a per-pixel offset, filters ~ 1 / 7; d is within
    (49 + 4) 2^-23 of sum |x| |w| + |bias| (49 fmaf and the bias add; S.elem_bound's count)."""
    rng = rng_of(800 + C)
    N_, H, W = cnb_shape(C)
    x = S.q_of(xdt)(rng.standard_normal((N_, H, W, C)) + rng.uniform(-1.0, 1.0, (N_, H, W, 1)))
    w = bf(rng.standard_normal((7, 7, C)) / 7.0)
    bias = (0.1 * rng.standard_normal(C)).astype(F32)
    wk = np.ascontiguousarray(w.transpose(2, 0, 1))[..., None]
    d, mag = S.conv_ref(x, wk, None, bias, None, 0, 1, 3, 1, C)
    ref, bound = post_ln_bound(d, (49 + 4) * U23 * mag, EPS, "bf16")
    for v in (x, w, bias, ref, bound):
        v.setflags(write=False)
    return x, w, bias, ref, bound


# ================================================================================================ mv_patch4_ln_fwd
# (B, H, K, split): H = 8 is one tile of 4 tokens; 3 x 28 x 28 is 147 tokens, a ragged second tile; K = 96 and 128; both weight forms
PATCH4_CASES = [(1, 8, 96, True), (1, 8, 128, False), (3, 28, 96, True), (3, 28, 96, False), (3, 28, 128, True), (5, 36, 128, False)]


def patch4_rows(x):
    """x [B][3][H][W] -> token rows [B Ho Wo][48], k = 16 c + 4 r + s (the (K, 3, 4, 4) filter flattened)."""
    B, _, H, W = x.shape
    return x.reshape(B, 3, H // 4, 4, W // 4, 4).transpose(0, 2, 4, 1, 3, 5).reshape(-1, 48)


@functools.lru_cache(maxsize=None)
def patch4_gauss(B, H, K, split):
    """(x fp32 image, hi, lo, b, gamma, beta, ref [M][K], bound).  The kernel rounds the image to bf16 (pack_bf2) and multiplies it
    with the hi and, if split, the lo bf16 term of the filter: the reference does the same in float64, so the only errors left are
    the fp32 accumulation of 48 (96) products and the bias add, (kred + 4) 2^-23 mag, pushed through the LayerNorm (post_ln_bound;
    the epilogue is fmaf(v * rstd, g, b): k_mul = 2, k_add = 1 as for patch_merge_ln_kernel), and the fp32 store."""
    rng = rng_of(900 + K + H)
    x = rng.random((B, 3, H, H), dtype=F32)
    x[0, :, :4, :4] = 0.0                                         # token 0: a black patch: d = bias, a variance of ~0.01 where eps shows
    w = (rng.standard_normal((K, 48)) / np.sqrt(48)).astype(F32)
    b = (0.1 * rng.standard_normal(K)).astype(F32)
    g, be = S.gauss_scale(rng, K), (0.1 * rng.standard_normal(K)).astype(F32)
    hi = bf(w)
    lo = bf(w - hi)
    rows = patch4_rows(bf(x)).astype(F64)
    weff = hi.astype(F64) + (lo.astype(F64) if split else 0.0)
    aw = np.abs(hi).astype(F64) + (np.abs(lo).astype(F64) if split else 0.0)
    d = rows @ weff.T + b.astype(F64)
    mag = np.abs(rows) @ aw.T + np.abs(b).astype(F64)
    ref, bound = post_ln_bound(d, ((96 if split else 48) + 4) * U23 * mag, EPS, "fp32", g, be, k_mul=2, k_add=1)
    for v in (x, hi, lo, b, g, be, ref, bound):
        v.setflags(write=False)
    return x, hi, lo, b, g, be, ref, bound


def emu_patch4_ln(x, hi, lo, b, g, be, split, eps=EPS, defect=None):
    """swin_stem_ln_kernel in float32: the image packed to bf16, one MFMA k-step per input channel (hi then lo), + bias, the
    statistics per lane half (channels 32 t + 8 g + 4 fh + i; float4 sums pairwise), v * rstd then fmaf with gamma, beta.  Defects:
    neighbour_stats (token m ^ 1), c_minus_1, no_eps, drop_chunk (the lo term of channel 1 is not accumulated; without lo: the hi
    term), trunc_pack (the image is truncated to bf16)."""
    K = hi.shape[0]
    rows = patch4_rows(S.store(x, "bf16", "trunc" if defect == "trunc_pack" else "rne"))
    M = rows.shape[0]
    acc = np.zeros((M, K), F32)
    for c in range(3):
        sl = slice(16 * c, 16 * c + 16)
        if not (defect == "drop_chunk" and c == 1 and not split):
            acc = acc + rows[:, sl] @ np.asarray(hi, F32)[:, sl].T
        if split and not (defect == "drop_chunk" and c == 1):
            acc = acc + rows[:, sl] @ np.asarray(lo, F32)[:, sl].T
    acc = acc + np.asarray(b, F32)
    v = acc.reshape(M, K // 32, 4, 2, 4)                          # [t][g][fh][i]
    s = np.zeros((M, 2), F32)
    for t in range(K // 32):
        for gg in range(4):
            s = s + ((v[:, t, gg, :, 0] + v[:, t, gg, :, 1]) + (v[:, t, gg, :, 2] + v[:, t, gg, :, 3]))
    mean = (s[:, 0] + s[:, 1]) * (F32(1) / F32(K))
    dv = v - mean[:, None, None, None, None]
    q = np.zeros((M, 2), F32)
    for t in range(K // 32):
        for gg in range(4):
            for i in range(4):
                q = q + dv[:, t, gg, :, i] * dv[:, t, gg, :, i]
    rstd = _finish_stats(q[:, 0] + q[:, 1], K, eps, defect)
    dvr = dv.reshape(M, K)
    if defect == "neighbour_stats":
        src = np.arange(M) ^ 1
        src = np.where(src < M, src, np.arange(M))
        dvr, rstd = acc - mean[src][:, None], rstd[src]
    with np.errstate(invalid="ignore", over="ignore"):
        y = ((dvr * rstd[:, None]).astype(F64) * np.asarray(g, F32).astype(F64) + np.asarray(be, F32).astype(F64)).astype(F32)
    return y


# ================================================================================================ mv_linear_lnout_fwd -> mv_linear_lnin_fwd
# The LayerNorm between two Linears folded into their epilogues (include/eqxvision_amd.h; igemm8.hip: ln_finalize, igemm_pipe.h:
# epilogue_rows_ln, merge_row_stats, epilogue_rows LNF 2).
#   producer   v = fp32(acc + shift + res); hi = bf16(v), lo = bf16(v - hi); per row and 64-column piece (sum, sum of squared deviations
#              from the piece's mean), four of them Chan-merged into one pair per 256 columns.
#   consumer   (mean, rstd) = Chan merge of the row's pairs, rstd = 1 / sqrtf(M2 / K + eps);
#              y = act(fmaf(rstd, acc, fmaf(-mean * rstd, colsum, b'))), acc = hi . W'^T in fp32 -- the operand is hi, NOT hi - mean.
# (M, D, Kp, N2, act, row_mean): shapes at which the 256 x 256 tile is the dispatch's choice (the pair exists nowhere else): D = 320 is
# two statistics pieces, the second one wave wide, M = 75 * 256 + 1 a last tile of one row; D = 512 two full pieces, rows offset by up to
# two standard deviations (the fold rounds y, not y - mean), GELU.
LNFOLD_CASES = [(75 * 256 + 1, 320, 256, 640, 0, 0.0), (75 * 256, 512, 512, 1024, 2, 2.0)]
LNFOLD_EPS = 1e-5
# The consumer's head-major form (tokens = 197, dh = 64) needs M % 197 == 0, which no row above has: 197 x 97 rows is the smallest
# multiple at which the producer (D = 320: 2 column tiles x 75 row tiles) and the consumer still take the 256 x 256 tile.  Its own
# table: tests/test_strict_entry_gpu.py runs the pair on it once (token-major and head-major), test_lnfold_pair keeps its two rows.
LNFOLD_TOKEN_CASE = (197 * 97, 320, 256, 640, 0, 0.0)
U24 = 2.0 ** -24
LNFOLD_STAT_OPS = 24          # roundings of the Chan merges beyond the N - 1 adds: per piece mu, d, the merge's d, d^2, 64 d^2, +, twice, / N


def lnfold_id(c):
    return f"M{c[0]}_D{c[1]}_K{c[2]}_N{c[3]}_act{c[4]}" + ("_offset" if c[5] else "")


@functools.lru_cache(maxsize=None)
def lnfold_data(M, D, Kp, N2, act, row_mean, seed=1000):
    """Operands as _cases.ln_fold_case draws them: (x bf16, w bf16, b, res fp32, W' bf16, colsum fp32, b' fp32)."""
    rng = rng_of(seed + D)
    x = bf(rng.standard_normal((M, Kp)))
    w = bf(rng.standard_normal((D, Kp)) / np.sqrt(Kp))
    b = (0.1 * rng.standard_normal(D)).astype(F32)
    res = rng.standard_normal((M, D)) * rng.uniform(0.5, 2.0, (M, 1))
    res = (res + row_mean * np.sqrt(2.0) * rng.uniform(-1, 1, (M, 1)) + rng.uniform(-0.3, 0.3, (M, 1))).astype(F32)
    x[5], res[5] = 0.0, (0.3 - b.astype(F64)).astype(F32)         # row 5: y = 0.3 to an fp32 ulp, a variance far below eps
    g, be = rng.uniform(0.5, 1.5, D).astype(F32), (0.1 * rng.standard_normal(D)).astype(F32)
    w2, b2 = (rng.standard_normal((N2, D)) / np.sqrt(D)).astype(F32), (0.1 * rng.standard_normal(N2)).astype(F32)
    wf = bf(w2 * g[None, :])
    cs = wf.astype(F64).sum(1).astype(F32)
    bfold = (b2.astype(F64) + w2.astype(F64) @ be.astype(F64)).astype(F32)
    for v in (x, w, b, res, wf, cs, bfold):
        v.setflags(write=False)
    return x, w, b, res, wf, cs, bfold


@functools.lru_cache(maxsize=None)
def lnout_ref(M, D, Kp, N2, act, row_mean):
    """(y_ref float64, e_y): the producer's fp32 value is within e_y = (Kp + 4) 2^-23 (|x| |w|^T + |b| + |res|) of y_ref."""
    x, w, b, res = lnfold_data(M, D, Kp, N2, act, row_mean)[:4]
    y, mag = S.gemm_ref(x, w, None, b, res, 0)
    e = (Kp + 4) * U23 * mag
    y.setflags(write=False), e.setflags(write=False)
    return y, e


def chan_merge64(stats, D):
    """stats [P][M][2] -> (mean, M2) per row in float64 (Chan's formula over the pieces of 256, the last one what is left of D)."""
    st = np.asarray(stats, F64)
    npc = np.array([min(256, D - 256 * j) for j in range(st.shape[0])], F64)[:, None]
    mean = st[:, :, 0].sum(0) / D
    return mean, (st[:, :, 1] + npc * (st[:, :, 0] / npc - mean[None, :]) ** 2).sum(0)


def check_lnout(hi, lo, stats, y_ref, e_y):
    """The producer's outputs, every element and every row (returns {name: info}, each with "ok" and "worst"):
      hi      a correct bf16 rounding of a value within e_y of y_ref: bf16(y_ref - e_y) <= hi <= bf16(y_ref + e_y) (rounding is monotone)
      lo      |lo| <= half a bf16 ulp of hi
      sum     |hi + lo - y_ref| <= e_y + half a bf16 ulp of (half a bf16 ulp of |y_ref| + e_y)      (lo's own rounding)
      mean    |Chan mean - mean(y_ref)| <= mean(e_y) + (D + 24) 2^-24 mean|y_ref|
      var     |M2 / D - var(y_ref)| <= 2 mean(|d| e_d) + mean(e_d^2) + (D + 24) 2^-24 var,   e_d = e_y + the mean's bound"""
    hi, lo, y, e = (np.asarray(v, F64) for v in (hi, lo, y_ref, e_y))
    D = y.shape[1]
    out = {}
    lo_b, hi_b = bf(y - e).astype(F64), bf(y + e).astype(F64)
    bad = (hi < lo_b) | (hi > hi_b)
    out["hi"] = {"ok": not bool(bad.any()), "worst": float(np.abs(hi - y).max()), "nviol": int(bad.sum())}
    out["lo"] = S.check_bound(np.abs(lo), np.zeros_like(lo), None, 0, "fp32", bound=half_ulp_out(np.abs(hi), "bf16"))
    hu = half_ulp_out(np.abs(y) + e, "bf16")
    out["sum"] = S.check_bound(hi + lo, y, None, 0, "fp32", bound=e + half_ulp_out(hu, "bf16"))
    mean_k, m2_k = chan_merge64(stats, D)
    mean_r, d = y.mean(1), y - y.mean(1, keepdims=True)
    var_r = (d * d).mean(1)
    e_mean = e.mean(1) + (D + LNFOLD_STAT_OPS) * U24 * np.abs(y).mean(1)
    e_d = e + e_mean[:, None]
    e_var = 2.0 * (np.abs(d) * e_d).mean(1) + (e_d * e_d).mean(1) + (D + LNFOLD_STAT_OPS) * U24 * var_r
    out["mean"] = S.check_bound(mean_k, mean_r, None, 0, "fp32", bound=e_mean)
    out["var"] = S.check_bound(m2_k / D, var_r, None, 0, "fp32", bound=e_var)
    return out


def lnin_ref_bound(hi, lo, wf, cs, bfold, act, eps=LNFOLD_EPS):
    """(ref, bound) of mv_linear_lnin_fwd given the planes it consumes -- the producer's own stored output, so the producer's error is
    not part of this bound.  Reference: float64 LayerNorm of the stream y2 = hi + lo (what the statistics describe, to 2^-17), times
    the bf16-rounded W', plus b'.  The kernel's effective operand is rstd (hi - mean); against n = (y2 - mean) / s it is off by
      operand     rstd |y2 - hi| <= half_ulp_bf16(hi) / s                                  (the issue's rstd (half_ulp(x_hi) @ |W'|^T))
      statistics  post_ln_bound(y2, e_s): ln_ref_bound's fp32 statistics and normalisation in any order with k_mean = 2 + 24 (the Chan
                  merges), and the sensitivity to e_s = half_ulp_bf16(half_ulp_bf16(hi)): the table is of v, and |v - y2| <= e_s
    both propagated through |W'|^T, plus
      accumulation (K + 7) 2^-23 (rstd |hi| |W'|^T + |mean rstd colsum| + |b'|): acc is of the UN-normalised hi (this is where a row
                  offset costs: |mean| / s times the colsum term), -mean * rstd, and the two fmaf
      colsum      |mean| / s times half an fp32 ulp of colsum (the host rounds the float64 sum once)
    then the activation and the bf16 store as for the other kernels (_through_act)."""
    hi, lo = np.asarray(hi, F64), np.asarray(lo, F64)
    K = hi.shape[1]
    aw = np.abs(wf).astype(F64)
    ref, bound = [], []
    for r0 in range(0, hi.shape[0], 4096):
        h, y2 = hi[r0:r0 + 4096], hi[r0:r0 + 4096] + lo[r0:r0 + 4096]
        mean = y2.mean(1, keepdims=True)
        s = np.sqrt(y2.var(1, keepdims=True) + float(F32(eps)))
        hu = half_ulp_out(np.abs(h), "bf16")
        n, e_stat = post_ln_bound(y2, half_ulp_out(hu, "bf16"), eps, "fp32", k_mean=2 + LNFOLD_STAT_OPS)
        e_n = hu / s + e_stat
        p = n @ wf.astype(F64).T + bfold.astype(F64)
        mag = (np.abs(h) @ aw.T) / s + np.abs(mean / s) * np.abs(cs).astype(F64) + np.abs(bfold).astype(F64)
        e_p = e_n @ aw.T + (K + 7) * U23 * mag + np.abs(mean / s) * half_ulp_out(np.abs(cs).astype(F64), "fp32")
        r, b = _through_act(p, e_p, act, "bf16")
        ref.append(r), bound.append(b)
    return np.concatenate(ref), np.concatenate(bound)


LNOUT_DEFECTS = ("trunc_hi", "lo_from_hi_twice", "stats_neighbour", "drop_chunk")
LNIN_DEFECTS = ("neighbour_stats", "c_minus_1", "no_eps", "drop_colsum", "drop_chunk", "trunc_pack")


def emu_lnout(x, w, b, res, defect=None):
    """The producer in float32 -> (hi, lo, stats [P][M][2]).  Defects: trunc_hi (hi truncated), lo_from_hi_twice (lo = bf16(v - hi)
    rounded from a v already rounded to bf16: always 0), stats_neighbour (row m ^ 1's pairs),
    drop_chunk (k-step 2 not accumulated)."""
    v = (_gemm32(x, w, 2 if defect == "drop_chunk" else None) + np.asarray(b, F32)) + np.asarray(res, F32)
    M, D = v.shape
    hi = S.bf16_truncate(v) if defect == "trunc_hi" else bf(v)
    lo = bf((hi if defect == "lo_from_hi_twice" else v) - hi)
    P = -(-D // 256)
    stats = np.zeros((P, M, 2), F32)
    for j in range(P):
        pc = v[:, 256 * j:256 * j + 256]
        nw = pc.shape[1] // 64
        w64 = pc.reshape(M, nw, 64)
        s = w64.sum(2, dtype=F32)
        mu = s * F32(1.0 / 64.0)
        dd = w64 - mu[:, :, None]
        q = (dd * dd).sum(2, dtype=F32)
        tot = s.sum(1, dtype=F32)
        mean = tot / F32(64 * nw)
        d = mu - mean[:, None]
        stats[j, :, 0], stats[j, :, 1] = tot, (q + F32(64.0) * d * d).sum(1, dtype=F32)
    if defect == "stats_neighbour":
        src = np.arange(M) ^ 1
        stats = stats[:, np.where(src < M, src, np.arange(M))]
    return hi, lo, stats


def emu_lnin(hi, stats, wf, cs, bfold, act, eps=LNFOLD_EPS, defect=None):
    """The consumer in float32: ln_finalize's Chan merge, then fmaf(rstd, acc, fmaf(-mean * rstd, colsum, b')), the activation, the bf16
    store.  Defects: neighbour_stats, c_minus_1, no_eps, drop_colsum (columns >= 128 lose the -mean rstd colsum term), drop_chunk,
    trunc_pack."""
    hi, st = np.asarray(hi, F32), np.asarray(stats, F32)
    M, K = hi.shape
    tot = st[:, :, 0].sum(0, dtype=F32)
    inv = F32(1) / F32(K)
    mean = tot * inv
    m2 = np.zeros(M, F32)
    for j in range(st.shape[0]):
        nj = F32(min(256, K - 256 * j))
        d = st[j, :, 0] / nj - mean
        m2 = m2 + (st[j, :, 1] + nj * d * d)
    var = m2 * (F32(1) / F32(K - 1) if defect == "c_minus_1" else inv)
    with np.errstate(divide="ignore", invalid="ignore"):
        rstd = (F32(1) / np.sqrt(var if defect == "no_eps" else var + F32(eps))).astype(F32)
    if defect == "neighbour_stats":
        src = np.arange(M) ^ 1
        src = np.where(src < M, src, np.arange(M))
        mean, rstd = mean[src], rstd[src]
    acc = _gemm32(hi, wf, 2 if defect == "drop_chunk" else None)
    c = np.array(cs, F32)
    if defect == "drop_colsum":
        c[128:] = 0
    with np.errstate(invalid="ignore", over="ignore"):
        y = rstd[:, None] * acc + ((-mean * rstd)[:, None] * c + np.asarray(bfold, F32))
        y = S.act32(y, {0: "none", 1: "relu", 2: "gelu_tanh"}[act])
    return S.store(y, "bf16", "trunc" if defect == "trunc_pack" else "rne")
