"""Strict instruments for mv_swin_block_attn_fwd (csrc/swin_block_attn.hip): y = x + proj(window_attention(qkv(LayerNorm(x)))) in one
launch, served by four kernels (KERNELS below).  Case table, data builders, CPU proofs, float64 references with per-element bounds,
and a numpy / float32 emulation of the kernels' order of operations with one switch per defect.  Used by
tests/test_strict_swinblock_gpu.py (the kernels) and tests/test_strict_swinblock_host.py (the CPU proof that the instruments see
each defect).  The kernel is the composition of a LayerNorm-into-GEMM kernel and a window-attention kernel, and so are the
instruments: the +-1 rows of tests/_strict_lngemm.py (prove_pm1) feed the select / tie / flat / mask softmax constructions of
tests/_strict_attn.py (build, prove).

Facts from the source the constructions rest on (csrc/swin_block_attn.hip, both kernel bodies):
  * the normalised row goes through pack_bf2((x - mean) * rstd), rstd = rsqrtf(q / C + eps); the LayerNorm affine is folded into
    the qkv weights by the host;
  * padded rows 49..63 are zeros (rstd = 0), so their q / k / v equal bqkv;
  * q, k, v are pack_bf2(acc + b) (v: f2bf(acc + b), transposed) into LDS (swin_win96: q stays in registers);
  * logit = fmaf(s, rsqrtf(32), bias), plus -100 where the mask regions of query and key differ; padded keys are masked only by
    the -1e30 columns ops.swin_block_attn_fragments writes into the 64 x 64 bias;
  * the maximum (exchanged between the two lane halves) is subtracted before __expf;
  * P is packed to bf16 before P . V; the sum is taken over the unrounded exponentials;
  * the attention output is pack_bf2(o * (1 / sum));
  * proj accumulates in fp32, then adds bp and the fp32 residual row (swin_win96: the accumulators START as the residual row, bp last);
  * the output is fp32, stored at the row the token was gathered from.
SUPPOSED, not in the source: __expf(0) = 1 exactly; __expf(t) = 0 exactly for t <= -128 (the -400 / -500 biases, the code gap of
181, -1e30); 1.f / 1.f = 1 and 1.f / 2.f = 0.5 exactly under the compiler's fast division.  A GPU that contradicts one shows as wrong
elements in every select (first two, fourth) or tie (last) case.

Instrument 1 -- exact, end to end.  Rows are m_r +- a_r (half the entries +, half -, a_r cycling through 1/4, 1, 4, 16 along the map's
rows so that neighbouring tokens differ by a factor >= 4; m_r = j a_r, |j| <= 8); G.prove_pm1 asserts at this kernel's eps that the
LDS fragment is exactly +-1.  From there every quantity is an integer (or a dyadic fraction) far below 2^24.
  form (a), select by bias.  Wq = Wk = 0 and bq = bk = 0: the logits are the bias alone.  V = Wv' n + bv' with Wv in {-1, 0, 1} (8 per
      row), gamma in {1, 2}, beta and bv integers, folded by ops._ln_fold: every token's v is an integer vector of magnitude <= 256,
      distinct inside its window and head (asserted).  Wp in {-1, 0, 1} (16 per row), bp integers.  The bias and the winners are
      A.build(kind, by_bias=True): 0 at the winner(s) and -400 elsewhere per head, the winners a permutation per head, tie pairs from
      one mask class (same side of the shift boundary in both axes) across the 32-key tile and across the lane halves.
      select, tie   y must EQUAL x + Wp v[pi(i)] + bp, or the tie's average (a multiple of 1/2; x a multiple of 1/4).
      flat          bias -400 everywhere (shifted maps: the query's region; the rest at -500): the region mean of v.  Bounded:
                    e_att = (49 + 8) 2^-24 |mean| + 2^-100, then steps 4 - 6 of instrument 2.
      mask          shifted maps only, bias 0: logits 0 inside the query's region, -100 outside; the region mean, bounded as flat.
  form (b), select by codes.  Channels 32 h .. 32 h + 31 of a token's +-1 row are [c8(sigma_h(t)) | -c8(sigma_h(t)) | c8(sigma_h(pi(t)))
      | -c8(sigma_h(pi(t)))] (c8: the low 8 bits as +-1; the complements keep the row balanced), sigma_h a permutation per head and pi a
      permutation per (image, window, head) inside the query's mask region.  Wk_h selects the first two blocks (+1 / -1) into A.codes'
      32-wide code of sigma_h(t), Wq_h the last two times g = A.gain(49, 32, rsqrt(32)) = 128; bias 0.  The winner's logit is
      128 * 32 * rsqrt(32) = 724, every other at least 2 * 128 * 4 * rsqrt(32) = 181 lower.  The q . k path, the scale, the mask and the
      head pairing decide the winner: a head that reads another head's q, k or v selects another token or another head's vector.
      LayerNorm affine: the identity.
  Every construction is proved on the CPU first (`_prove`): A.prove on float64 logits of the STORED operands (winners equal, gap >=
  128 -- 100 for flat / mask --, products below 2^24), S.prove_exact (integers, |v| <= 256, sums below 2^24, every reduction index
  used, non-zero outputs), v distinct per window and head.

Instrument 2 -- per-element bound on Gaussian rows (G.gauss_rows: per-token scale and offset, every seventh row with a common offset
of 50 of its standard deviations, row 5 constant: variance 0), gamma in [0.5, 1.5] and beta folded by ops._ln_fold.  The reference is
float64 ON THE OPERANDS THE KERNEL GETS (bf16-rounded folded weights, fp32 biases).  u23 = 2^-23, h(x) the half ulp of a bf16 value:
  1. n, e_ln = N.ln_ref_bound(x, no affine, bf16)           t = n W'^T + b'     mag1 = (|n| + e_ln) |W'|^T + |b'|
     pre = e_ln |W'|^T + (C + 4) u23 mag1                                        S.elem_bound's accumulation term
  2. e_t = pre + h(|t| + pre)                                                    the bf16 packs of q, k, v: e_q, e_k, e_v
  3. eL_ij = scale (e_q_i . |k_j| + |q_i| . e_k_j + e_q_i . e_k_j)              what the operand errors do to a logit
     g_ij = exp(eL_ij) - 1: an exponential is off by a factor 1 + d_j, |d_j| <= g_j (the subtracted maximum cancels between numerator
     and denominator).  With p the float64 probabilities and out = p v, sum_j p_j (v_j - out) = 0 gives, without linearising,
         out' - out = (sum_j p_j d_j (v_j - out) + sum_j p_j (1 + d_j) dv_j) / sum_j p_j (1 + d_j)
         e_in = (sum_j p_j (g_j |v_j| + (1 + g_j) e_v_j) + |out| r) / lo,     r = sum_j p_j g_j,  lo = sum_j p_j exp(-eL_j)
     e_p = sum_j h(pe_j) (|v_j| + e_v_j) / sum_j pe_j                            A.p_round_mag: P rounded to bf16
     e_att = e_in + (e_p + A.n_ops(S, 64, 32) 2^-24 sum_j p_j (|v_j| + e_v_j)) (1 + max g) / lo
     S = max_j (scale (|q| + e_q) . (|k| + e_k) + |bias| + |mask|); 64 keys: the sums run over the padded ones too.
  4. e_o = e_att + h(|out| + e_att)                                              the bf16 pack of the attention output
  5. y = x + o Wp^T + bp     mag2 = (|o| + e_o) |Wp|^T + |bp| + |x|     e_2 = e_o |Wp|^T + (C + 5) u23 mag2
     (C + 4, and one more rounding for the residual; swin_win96's accumulators start as the residual: |x| is inside mag2)
  6. bound = e_2 + half_ulp_fp32(|y| + e_2)                                      the fp32 store
No factor is chosen by eye.  The rounding-bias rule is NOT applied: the project's condition is a bf16 output with >= 4096 eligible
elements, and this output is fp32 -- its store rounds nothing that a mean over elements could show (N.judge decides the same from the
reference alone).

Instrument 1c ("b-soft") -- form (b)'s rows at gain 1: the logits (32 - 8 * differing bits) * rsqrt(32) <= 5.7 make a real softmax
over EXACT integer q, k, v.  Reference float64 on them; bound e_att = e_p + A.n_ops(S, 64, 32) 2^-24 sum_j p_j |v_j| (no operand
error), then steps 4 - 6.  It is the instrument that sees a wrong scale: the exact ones cannot (below).

Worst |err| / bound of the honest emulation on the CPU, map 14 x 21, shift (2, 5), B = 1 (tests/test_strict_swinblock_host.py prints
them with -s); a-select, a-tie and b are bit-equal at all four kernels:
    kernel                 a-flat  a-mask  b-soft  gauss
    swin_block_attn_c384   0.595   0.595   0.447   0.001
    swin_block_attn_c192   0.785   0.785   0.349   0.002
    swin_block_attn_c96    0.676   0.676   0.390   0.004
    swin_win96             0.676   0.676   0.390   0.004
The Gaussian bound propagates the half ulps of the q / k packs in absolute value over 96 .. 384 terms and then through the
exponentials, while the errors add like a random walk: the honest ratio is 0.001 .. 0.006, so on its own it rejects only defects
that move an output grossly (neighbour_stats, roll_back_wrong, res_rolled, no_half_exchange, window_pair_swap).  The exact
instruments and b-soft are what reject the rest.
Seeded defects (DEFECTS) and the instruments that reject them in the emulation at all four kernels unless said otherwise (a-*: form
(a) select, tie, flat, mask); `cmp`: the former `_cmp(got, ref, 1e-2)` lets the defect through on the same Gaussian data:
    neighbour_stats         a-* b b-soft gauss
    c_minus_1               a-select a-tie b at C = 96 and 192 (+-1 becomes 0.9961)                                           cmp
                            NOT REJECTED at swin_block_attn_c384: sqrt(383 / 384) leaves +-1 where it is in bf16 and the Gaussian
                            bound is far too wide (the midpoint rows of tests/_strict_lngemm.py, instrument 1b, are not composed here)
    trunc_pack              a-* b b-soft (the a_r = 1/4 rows: 0.99992 truncates to 0.9961)                                    cmp
    drop_wbeta              a-* (form (b) has the identity affine)                                                            cmp
    swap_hw, swap_shift     a-* b b-soft (other tokens share a window, other regions)
    roll_back_wrong         a-* b b-soft gauss            res_rolled   a-* b b-soft gauss
    mask_region_off_by_one  a-tie a-flat a-mask b-soft (b where a winner sits across the moved boundary)
    unmasked_pad            a-* (logit 0 ties with or beats the winner; the padded v is bv'); b cannot (winner at 724)        cmp
    pad_rows_not_zero       NOT REJECTED, by design: the padded keys' probabilities are exactly 0 through the -1e30 columns and padded
                            queries are never stored, so finite values in those rows cannot reach an output                   cmp
    head_cross              a-* b b-soft                  v_key_order  a-select b b-soft                                      cmp (but C = 192)
    no_half_exchange        a-* b b-soft gauss
    window_pair_swap        a-* b b-soft gauss at NWIN = 2 (swin_block_attn_c192, _c96); n/a at one window per workgroup
    scale_off (x 1.02)      b-soft only: 1.02 * 724 keeps every gap of b, form (a) has s = 0                                  cmp
    scale_half (x 0.5)      b-soft (and b at C = 384): a gap of 90 is still exp(-90) = 0 next to integers                     cmp
    drop_proj_bias          a-* b b-soft                                                                                      cmp
    truncate_p              NOT REJECTED: every exact P is 0 or 1, and on Gaussian or code-selected v the error's sign is random;
                            tests/_strict_attn.py sees it as the rounding BIAS of a bf16 output, which this kernel does not have  cmp
(tests/test_strict_swinblock_host.py prints this table and asserts the claims the design rests on.)
"""
from __future__ import annotations

import functools
import types

import numpy as np

from tests import _strict as S
from tests import _strict_attn as A
from tests import _strict_lngemm as G
from tests import _strict_norm as N

F32, F64 = np.float32, np.float64
EPS = 1e-5
U23 = 2.0 ** -23
WS, NTOK, DH, NPAD = 7, 49, 32, 64
SENTINEL = S.SENTINEL
SCALE32 = F32(1.0 / np.sqrt(32.0))          # rsqrtf(32.0f)

# kernel -> (C, windows per workgroup, flags, the LayerNorm's order of summation in G._normalise)
KERNELS = {"swin_block_attn_c384": (384, 1, (), "stream"), "swin_block_attn_c192": (192, 2, (), "stream"),
           "swin_block_attn_c96": (96, 2, ("swin_c96_shared",), "stream"), "swin_win96": (96, 1, (), "half")}
# (B, Hf, Wf, shh, shw).  14 x 14: 4 windows, two workgroups per image at NWIN = 2; 14 x 21 / 21 x 14: 6 windows, nWw != nWh, the second
# window of a pair in another window row (21 x 14: windows 1 | 2); 21 x 21: 9 windows, the interior one with region 0 throughout
GEOMS = [(2, 14, 14, 0, 0), (2, 14, 14, 3, 3), (2, 14, 21, 0, 0), (2, 14, 21, 3, 3), (2, 14, 21, 2, 5),
         (2, 21, 14, 0, 0), (2, 21, 14, 3, 3), (2, 21, 14, 2, 5)]
GEOMS_ODD = [(2, 21, 21, 0, 0), (2, 21, 21, 3, 3)]            # an odd window count: NWIN = 2 must refuse it
CASES = [(k, g) for k in KERNELS for g in GEOMS + (GEOMS_ODD if KERNELS[k][1] == 1 else [])]
HOST_GEOM = (1, 14, 21, 2, 5)                                 # the emulation's case: rectangular, unequal shifts, three window pairs
KINDS_A = ("select", "tie", "flat", "mask")


def case_id(c):
    k, (B, Hf, Wf, shh, shw) = c
    return f"{k}-B{B}_{Hf}x{Wf}_s{shh}{shw}"


# ================================================================================================ geometry (numpy restatement)
def tok_index(B, Hf, Wf, shh, shw):
    """(B, nW, 49): the row of x that window token (window, t) is -- the reference's roll by (-shh, -shw) and window partition."""
    idx = np.arange(B * Hf * Wf).reshape(B, Hf, Wf)
    if shh + shw > 0:
        idx = np.roll(idx, (-shh, -shw), axis=(1, 2))
    return idx.reshape(B, Hf // WS, WS, Wf // WS, WS).transpose(0, 1, 3, 2, 4).reshape(B, -1, NTOK)


def region_map(Hf, Wf, shh, shw, off_by_one=False):
    """(nW, 49) region ids of the rolled map, by the reference's per-axis slices: blocks of (L - ws, ws - shift, shift) rows and
    columns, id = 3 * row block + column block; all zero on an un-shifted map.  off_by_one: the defect (the last boundary one later)."""
    nW = (Hf // WS) * (Wf // WS)
    if shh + shw == 0:
        return np.zeros((nW, NTOK), np.int64)

    def blocks(L, s):
        e = L - s + (1 if off_by_one and s > 0 else 0)
        return ((0, L - WS), (L - WS, e), (e, L))
    m = np.zeros((Hf, Wf), np.int64)
    for i, a in enumerate(blocks(Hf, shh)):
        for j, b in enumerate(blocks(Wf, shw)):
            m[a[0]:a[1], b[0]:b[1]] = 3 * i + j
    return m.reshape(Hf // WS, WS, Wf // WS, WS).transpose(0, 2, 1, 3).reshape(nW, NTOK)


def mask_classes(shh, shw):
    """(49,) which side of the shift boundary a window token is on, per axis: tokens of one class share a region in every window."""
    t = np.arange(NTOK)
    return ((t // WS) >= WS - shh) * 2 + ((t % WS) >= WS - shw) if shh + shw > 0 else np.zeros(NTOK, np.int64)


def to_groups(rows, idx, heads):
    """(M, heads * 32) -> (B nW heads, 49, 32), groups ordered (image, window, head)."""
    B, nW, _ = idx.shape
    w = rows[idx.reshape(-1)].reshape(B, nW, NTOK, heads, DH)
    return np.ascontiguousarray(w.transpose(0, 1, 3, 2, 4)).reshape(B * nW * heads, NTOK, DH)


def from_groups(o, idx, heads):
    B, nW, _ = idx.shape
    w = o.reshape(B, nW, heads, NTOK, DH).transpose(0, 1, 3, 2, 4).reshape(B * nW * NTOK, heads * DH)
    out = np.empty_like(w)
    out[idx.reshape(-1)] = w
    return out


def fold(w, b, gamma, beta):
    """The project's own fold of a LayerNorm affine into the Linear behind it (ops._ln_fold)."""
    from eqxvision_amd import ops
    ns = types.SimpleNamespace
    return ops._ln_fold(ns(weight=np.asarray(w, F32), bias=np.asarray(b, F32)), ns(weight=np.asarray(gamma, F32), bias=np.asarray(beta, F32)))


# ================================================================================================ steps 4 - 6, shared
def tail_bound(o, e_o_pre, wp, bp, x):
    """(y, bound) of y = x + bf16(o) Wp^T + bp for an attention output known to e_o_pre before its bf16 pack."""
    C = x.shape[1]
    e_o = e_o_pre + S.half_ulp_out(np.abs(o) + e_o_pre, "bf16")
    wp64, awp = np.asarray(wp, F64), np.abs(np.asarray(wp, F64))
    x64, bp64 = np.asarray(x, F64), np.asarray(bp, F64)
    y = x64 + o @ wp64.T + bp64
    mag2 = (np.abs(o) + e_o) @ awp.T + np.abs(bp64) + np.abs(x64)
    e2 = e_o @ awp.T + (C + 5) * U23 * mag2
    return y, e2 + S.half_ulp_out(np.abs(y) + e2, "fp32")


def _freeze(op):
    for v in op.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return op


def _rows_from_signs(sg, Wf, rng):
    """x = m_r + a_r sg: a_r cycles through 1/4, 1, 4, 16 along the flat rows of the map.  Wf is 14 or 21, no multiple of 4, so the
    tokens left and right (one step of the cycle) and above and below (Wf % 4 = 2 or 1 steps) all differ by a factor >= 4."""
    M = sg.shape[0]
    assert Wf % 4 != 0
    a = np.array((0.25, 1.0, 4.0, 16.0))[np.arange(M) % 4]
    m = rng.integers(-8, 9, M) * a
    return (m[:, None] + a[:, None] * sg).astype(F32), a, m


def _ternary(rng, rows, kred, nnz):
    """G._ternary, with a +-1 put into every reduction index and every row it left empty."""
    w = G._ternary(rng, rows, kred, nnz)
    for c in np.flatnonzero(~(w != 0).any(0)):
        w[rng.integers(rows), c] = rng.choice(np.array([-1.0, 1.0], F32))
    for r in np.flatnonzero(~(w != 0).any(1)):
        w[r, rng.integers(kred)] = rng.choice(np.array([-1.0, 1.0], F32))
    return w


def _prove(name, op, p, extra, v, o, exact):
    A.prove(p, extra)
    C = op["wp"].shape[0]
    vi = np.rint(v)
    assert np.array_equal(vi, v) and np.abs(v).max() <= S.BF16_INT_MAX, f"{name}: v is not an integer vector of magnitude <= 256"
    assert np.array_equal(S.bf(op["wqkv"]), op["wqkv"]) and np.array_equal(S.bf(op["wp"]), op["wp"]), f"{name}: weights are not bf16 values"
    for g in range(v.shape[0]):
        assert len({r.tobytes() for r in v[g]}) == NTOK, f"{name}: two tokens of group {g} share their v"
    S._prove_coverage(name, [op["wqkv"][2 * C:], op["wp"]])
    x64 = op["x"].reshape(-1, C).astype(F64)
    mag2 = np.abs(o) @ np.abs(op["wp"]).astype(F64).T + np.abs(op["bp"]) + np.abs(x64)
    if exact:
        S.prove_exact(name, op["ref"], mag2, [op["wp"]], stored=[v], hidden=[o], out="fp32", frac_bits=2, hidden_max=4 * S.BF16_INT_MAX)
    assert ((op["ref"] - x64) != 0).mean() > 0.5, f"{name}: the attention half contributes nothing to most outputs"


def _geometry(kernel, geom):
    C = KERNELS[kernel][0]
    B, Hf, Wf, shh, shw = geom
    heads = C // DH
    idx = tok_index(B, Hf, Wf, shh, shw)
    reg = region_map(Hf, Wf, shh, shw)
    nW = reg.shape[0]
    greg = np.broadcast_to(reg[None, :, None], (B, nW, heads, NTOK)).reshape(B * nW * heads, NTOK)
    return C, heads, idx, reg, greg, B * Hf * Wf


# ================================================================================================ instrument 1, form (a)
@functools.lru_cache(maxsize=None)
def exact_a(kernel, geom, kind, seed=900):
    """The operands and the reference of form (a).  Returns a dict: x (M, C), wqkv (3C, C) / bqkv (3C,) folded, bqkv_raw (without W beta),
    wp, bp, bias (heads, 49, 49), ref (M, C) float64, bound (None: bit equality)."""
    C, heads, idx, reg, greg, M = _geometry(kernel, geom)
    B, Hf, Wf, shh, shw = geom
    name = f"swinblock/a/{kind}/{case_id((kernel, geom))}"
    assert kind != "mask" or shh + shw > 0, "mask: shifted maps only"
    rng = S.rng_of(seed + C + 7 * Hf + Wf + shh)
    sg = rng.permuted(np.tile(np.repeat(np.array([1.0, -1.0], F32), C // 2), (M, 1)), axis=1)
    x, a, m = _rows_from_signs(sg, Wf, rng)
    G.prove_pm1(name, x, sg, a, m, EPS)
    w, b = np.zeros((3 * C, C), F32), np.zeros(3 * C, F32)
    w[2 * C:], b[2 * C:] = _ternary(rng, C, C, 8), S.int_tensor(rng, (C,), 8)
    gamma, beta = rng.choice(np.array([1.0, 2.0], F32), C), S.int_tensor(rng, (C,), 2)
    wf, bfold = fold(w, b, gamma, beta)
    wp, bp = _ternary(rng, C, C, 16), S.int_tensor(rng, (C,), 8)
    Gn = greg.shape[0]
    p = A.build(kind, Gn, NTOK, DH, float(DH) ** -0.5, seed + 1 + C + shh + 3 * shw, regions=greg, by_bias=True,
                classes=mask_classes(shh, shw), heads=heads)
    t = sg.astype(F64) @ wf.astype(F64).T + bfold.astype(F64)                     # from the STORED operands
    q, k, v = (to_groups(t[:, i * C:(i + 1) * C], idx, heads) for i in range(3))
    extra = A.swin_extra(p["bias"], reg, heads, B)
    win = p["win"]
    o = from_groups((win.astype(F64) @ v) / win.sum(-1, keepdims=True), idx, heads)
    op = {"kind": kind, "geom": geom, "x": x.reshape(B, Hf, Wf, C), "wqkv": wf, "bqkv": bfold, "bqkv_raw": b, "wp": wp, "bp": bp,
          "bias": p["bias"]}
    if kind in ("select", "tie"):
        op["ref"], op["bound"] = x.astype(F64) + o @ wp.astype(F64).T + bp, None
    else:
        op["ref"], op["bound"] = tail_bound(o, (NTOK + 8) * 2.0 ** -24 * np.abs(o) + 2.0 ** -100, wp, bp, x)
    _prove(name, op, {"kind": kind, "q": q, "k": k, "v": v, "win": win, "scale": float(DH) ** -0.5}, extra, v, o, op["bound"] is None)
    return _freeze(op)


# ================================================================================================ instrument 1, form (b)
def _c8(j):
    return np.where((np.asarray(j)[..., None] >> np.arange(8)) & 1, 1.0, -1.0).astype(F32)


@functools.lru_cache(maxsize=None)
def exact_b(kernel, geom, soft=False, seed=950):
    """Form (b): the codes ride in the +-1 rows, Wk / Wq select them; one permutation per (image, window, head) inside the mask region.
    soft: the gain is 1, so that the logits (32 - 8 * differing bits) * rsqrt(32) <= 5.7 make a real softmax over EXACT q, k, v: the
    reference is float64 on them and the bound is the attention's own arithmetic (e_p and n_ops, no operand error), then steps 4 - 6."""
    C, heads, idx, reg, greg, M = _geometry(kernel, geom)
    B, Hf, Wf, shh, shw = geom
    nW = reg.shape[0]
    name = f"swinblock/b/{case_id((kernel, geom))}"
    rng = S.rng_of(seed + C + 7 * Hf + Wf + shh)
    pi = A._perm_in_regions(rng, greg).reshape(B, nW, heads, NTOK)
    sigma = np.stack([rng.permutation(NTOK) for _ in range(heads)])                # (heads, 49)
    kc = _c8(np.broadcast_to(sigma[None, None], (B, nW, heads, NTOK)))             # (B, nW, heads, 49, 8)
    qc = _c8(np.take_along_axis(np.broadcast_to(sigma[None, None], (B, nW, heads, NTOK)), pi, -1))
    blk = np.concatenate([kc, -kc, qc, -qc], -1)                                   # (B, nW, heads, 49, 32)
    sg = np.empty((M, C), F32)
    sg[idx.reshape(-1)] = blk.transpose(0, 1, 3, 2, 4).reshape(M, C)
    x, a, m = _rows_from_signs(sg, Wf, rng)
    G.prove_pm1(name, x, sg, a, m, EPS)
    g = 1.0 if soft else A.gain(NTOK, DH, float(DH) ** -0.5)
    w, b = np.zeros((3 * C, C), F32), np.zeros(3 * C, F32)
    d = np.arange(DH)
    for h in range(heads):
        w[C + DH * h + d, DH * h + (d % 8) + np.where(d < 16, 0, 8)] = np.where(d < 16, 1.0, -1.0)           # k = codes[sigma(t)]
        w[DH * h + d, DH * h + 16 + (d % 8) + np.where(d < 16, 0, 8)] = g * np.where(d < 16, 1.0, -1.0)      # q = g codes[sigma(pi(t))]
    w[2 * C:], b[2 * C:] = _ternary(rng, C, C, 8), S.int_tensor(rng, (C,), 8)
    wp, bp = _ternary(rng, C, C, 16), S.int_tensor(rng, (C,), 8)
    t = sg.astype(F64) @ w.astype(F64).T + b.astype(F64)
    q, k, v = (to_groups(t[:, i * C:(i + 1) * C], idx, heads) for i in range(3))
    codes = A.codes(NTOK, DH).astype(F64)
    assert np.array_equal(k.reshape(B, nW, heads, NTOK, DH), np.broadcast_to(codes[sigma][None, None], (B, nW, heads, NTOK, DH)))
    win = np.zeros((B * nW * heads, NTOK, NTOK), bool)
    win[np.arange(win.shape[0])[:, None], np.arange(NTOK)[None, :], pi.reshape(-1, NTOK)] = True
    bias = np.zeros((heads, NTOK, NTOK), F32)
    if soft:
        sc = float(DH) ** -0.5
        extra = A.swin_extra(bias, reg, heads, B)
        assert np.abs(v).max() <= S.BF16_INT_MAX and np.array_equal(np.rint(v), v), name
        L = q @ k.transpose(0, 2, 1) * sc + extra
        smag = (sc * (np.abs(q) @ np.abs(k).transpose(0, 2, 1)) + np.abs(extra)).max(-1, keepdims=True)
        pe = np.exp(L - L.max(-1, keepdims=True))
        D = pe.sum(-1, keepdims=True)
        e_att = (S.half_ulp_out(pe, "bf16") @ np.abs(v)) / D + A.n_ops(smag, NPAD, DH) * 2.0 ** -24 * ((pe / D) @ np.abs(v))
        op = {"kind": "soft", "geom": geom, "x": x.reshape(B, Hf, Wf, C), "wqkv": w, "bqkv": b, "bqkv_raw": b, "wp": wp, "bp": bp, "bias": bias}
        op["ref"], op["bound"] = tail_bound(from_groups((pe / D) @ v, idx, heads), from_groups(e_att, idx, heads), wp, bp, x)
        S._prove_coverage(name, [w[:2 * C], w[2 * C:], wp])
        return _freeze(op)
    o = from_groups(win.astype(F64) @ v, idx, heads)
    op = {"kind": "codes", "geom": geom, "x": x.reshape(B, Hf, Wf, C), "wqkv": w, "bqkv": b, "bqkv_raw": b, "wp": wp, "bp": bp, "bias": bias,
          "ref": x.astype(F64) + o @ wp.astype(F64).T + bp, "bound": None}
    _prove(name, op, {"kind": "select", "q": q, "k": k, "v": v, "win": win, "scale": float(DH) ** -0.5},
           A.swin_extra(bias, reg, heads, B), v, o, True)
    S._prove_coverage(name, [w[:2 * C]])                           # every channel feeds a q or a k row
    return _freeze(op)


# ================================================================================================ instrument 2
@functools.lru_cache(maxsize=None)
def gauss(kernel, geom, seed=1000):
    C, heads, idx, reg, greg, M = _geometry(kernel, geom)
    B, Hf, Wf, shh, shw = geom
    x = G.gauss_rows(M, C, "fp32", seed + C + Hf)
    rng = S.rng_of(seed + 1 + C + 7 * Hf + Wf + shh)
    gam, be = rng.uniform(0.5, 1.5, C).astype(F32), (0.1 * rng.standard_normal(C)).astype(F32)
    wq, bq = (rng.standard_normal((3 * C, C)) / np.sqrt(C)).astype(F32), (0.1 * rng.standard_normal(3 * C)).astype(F32)
    wp, bp = S.bf(rng.standard_normal((C, C)) / np.sqrt(C)), (0.1 * rng.standard_normal(C)).astype(F32)
    bias = (0.5 * rng.standard_normal((heads, NTOK, NTOK))).astype(F32)
    wf, bfold = fold(wq, bq, gam, be)
    op = {"kind": "gauss", "geom": geom, "x": x.reshape(B, Hf, Wf, C), "wqkv": S.bf(wf), "bqkv": bfold.astype(F32), "bqkv_raw": bq, "wp": wp,
          "bp": bp, "bias": bias}
    op["ref"], op["bound"] = gauss_ref_bound(op)
    return _freeze(op)


def gauss_ref_bound(op):
    """(ref, bound), both (M, C) float64: the module docstring's steps 1 - 6."""
    B, Hf, Wf, shh, shw = op["geom"]
    C = op["wp"].shape[0]
    heads = C // DH
    idx, reg = tok_index(B, Hf, Wf, shh, shw), region_map(Hf, Wf, shh, shw)
    x = op["x"].reshape(-1, C)
    w64, b64 = op["wqkv"].astype(F64), op["bqkv"].astype(F64)
    n, e_ln = N.ln_ref_bound(x, None, None, None, EPS, "bf16")
    t = n @ w64.T + b64
    mag1 = (np.abs(n) + e_ln) @ np.abs(w64).T + np.abs(b64)
    pre = e_ln @ np.abs(w64).T + (C + 4) * U23 * mag1
    e_t = pre + S.half_ulp_out(np.abs(t) + pre, "bf16")
    q, k, v = (to_groups(t[:, i * C:(i + 1) * C], idx, heads) for i in range(3))
    eq, ek, ev = (to_groups(e_t[:, i * C:(i + 1) * C], idx, heads) for i in range(3))
    sc = float(DH) ** -0.5
    extra = A.swin_extra(op["bias"], reg, heads, B)
    kT, ekT = k.transpose(0, 2, 1), ek.transpose(0, 2, 1)
    L = q @ kT * sc + extra
    eL = sc * (eq @ np.abs(kT) + np.abs(q) @ ekT + eq @ ekT)
    smag = (sc * ((np.abs(q) + eq) @ (np.abs(kT) + ekT)) + np.abs(extra)).max(-1, keepdims=True)
    pe = np.exp(L - L.max(-1, keepdims=True))
    D = pe.sum(-1, keepdims=True)
    p = pe / D
    g = np.expm1(eL)
    r = (p * g).sum(-1, keepdims=True)
    lo = (p * np.exp(-eL)).sum(-1, keepdims=True)                  # the perturbed denominator is at least lo times the true one
    av = np.abs(v) + ev
    out = p @ v
    e_in = ((p * g) @ np.abs(v) + (p * (1.0 + g)) @ ev + np.abs(out) * r) / lo
    e_p = (S.half_ulp_out(pe, "bf16") @ av) / D
    grow = (1.0 + g.max(-1, keepdims=True)) / lo
    e_att = e_in + (e_p + A.n_ops(smag, NPAD, DH) * 2.0 ** -24 * (p @ av)) * grow
    return tail_bound(from_groups(out, idx, heads), from_groups(e_att, idx, heads), op["wp"], op["bp"], x)


# ================================================================================================ the instruments of one case
def instruments(kernel, geom):
    """[(name, operands)] of a (kernel, geometry): a-select, a-tie, a-flat, a-mask (shifted), b, b-soft, gauss."""
    shifted = geom[3] + geom[4] > 0
    out = [("a-" + kd, exact_a(kernel, geom, kd)) for kd in KINDS_A if kd != "mask" or shifted]
    return out + [("b", exact_b(kernel, geom)), ("b-soft", exact_b(kernel, geom, True)), ("gauss", gauss(kernel, geom))]


def check(op, got):
    """tests/_strict-style info: bit equality where the operands carry no bound, else every element within it (N.judge; the bias
    rule does not apply to an fp32 output).  `left`: sentinel values left inside the output."""
    got = np.asarray(got, F64).reshape(op["ref"].shape)
    if op["bound"] is None:
        info = S.check_exact(got, op["ref"])
        info["worst"] = 0.0 if info["ok"] else float("inf")
        info["left"] = int(((got == SENTINEL) & (op["ref"] != SENTINEL)).sum())
    else:
        info, bias = N.judge(got, op["ref"], op["bound"], "fp32")
        assert bias["n_bias"] == 0                                 # fp32 output: the rule does not apply
        info["left"] = int(((got == SENTINEL) & (np.abs(op["ref"] - SENTINEL) > op["bound"])).sum())
    info["ok"] = bool(info["ok"] and info["left"] == 0)
    return info


# ================================================================================================ emulation
DEFECTS = ("neighbour_stats", "c_minus_1", "trunc_pack", "drop_wbeta", "swap_hw", "swap_shift", "roll_back_wrong", "res_rolled",
           "mask_region_off_by_one", "unmasked_pad", "pad_rows_not_zero", "head_cross", "v_key_order", "no_half_exchange",
           "window_pair_swap", "scale_off", "scale_half", "drop_proj_bias", "truncate_p")
NOT_REJECTED = {"pad_rows_not_zero": "padded keys have probability exactly 0 (-1e30) and padded queries are never stored",
                "truncate_p": "every exact P is 0 or 1; on Gaussian v the error's sign is random and an fp32 output has no bias rule"}

NOT_REJECTED_AT = {("swin_block_attn_c384", "c_minus_1"): "sqrt(383 / 384) leaves +-1 where it is in bf16; far inside the Gaussian bound"}


def emulate(kernel, op, defect=None):
    """float32 model of the kernels' order of operations (module docstring, "facts"); returns y (M, C) float32 with the sentinel
    wherever nothing was stored.  One defect per switch:
      neighbour_stats, c_minus_1, trunc_pack   G._normalise's (trunc_pack: every bf16 pack truncates)
      drop_wbeta               folded bias channels >= 128 without W beta
      swap_hw / swap_shift     Hf and Wf / shh and shw exchanged in the gather, the mask and the scatter
      roll_back_wrong          the output rows stored at the rolled position       res_rolled   the residual read there
      mask_region_off_by_one   region_map's switch       unmasked_pad   key 49 keeps bias 0
      pad_rows_not_zero        the padded rows carry token 0's normalised row
      head_cross               q of head h with k and v of head h + 1
      v_key_order              keys 32 and 33 exchanged on the V side only
      no_half_exchange         1 / sum from the keys of one lane half only (A.emulate's)
      window_pair_swap         NWIN = 2: the two windows of a workgroup trade attention outputs
      scale_off / scale_half   scale * 1.02 / * 0.5      drop_proj_bias   bp missing on channels 32 .. 63
      truncate_p               P truncated to bf16"""
    assert defect is None or defect in DEFECTS, defect
    C, nwin, _, lnkind = KERNELS[kernel]
    B, Hf, Wf, shh, shw = op["geom"]
    heads = C // DH
    mode = "trunc" if defect == "trunc_pack" else "rne"
    gH, gW = (Wf, Hf) if defect == "swap_hw" else (Hf, Wf)
    sh, sw = (shw, shh) if defect == "swap_shift" else (shh, shw)
    idx = tok_index(B, gH, gW, sh, sw)
    idx0 = tok_index(B, gH, gW, 0, 0)
    nW = idx.shape[1]
    reg = region_map(gH, gW, sh, sw, off_by_one=defect == "mask_region_off_by_one")
    rows = np.asarray(op["x"], F32).reshape(-1, C)
    flat = idx.reshape(-1)
    xw = rows[flat]
    n = G._normalise(xw, EPS, lnkind, defect)
    bq = np.array(op["bqkv"], F32)
    if defect == "drop_wbeta":
        bq[128:] = op["bqkv_raw"][128:]
    with np.errstate(invalid="ignore", over="ignore", under="ignore", divide="ignore"):
        t = S.store(G._gemm32(n, op["wqkv"]) + bq, "bf16", mode).reshape(B, nW, NTOK, 3 * C)
        t64 = np.empty((B, nW, NPAD, 3 * C), F32)
        t64[:, :, :NTOK] = t
        t64[:, :, NTOK:] = t[:, :, :1] if defect == "pad_rows_not_zero" else S.store(bq, "bf16", mode)
        q, k, v = (t64[..., i * C:(i + 1) * C].reshape(B, nW, NPAD, heads, DH).transpose(0, 1, 3, 2, 4) for i in range(3))
        if defect == "head_cross":
            k, v = np.roll(k, -1, axis=2), np.roll(v, -1, axis=2)
        b64 = np.zeros((heads, NPAD, NPAD), F32)
        b64[:, :, NTOK:] = -1e30
        b64[:, :NTOK, :NTOK] = op["bias"]
        if defect == "unmasked_pad":
            b64[:, :, NTOK] = 0.0
        sc = F64(SCALE32) * (1.02 if defect == "scale_off" else 0.5 if defect == "scale_half" else 1.0)
        s = q @ k.transpose(0, 1, 2, 4, 3)                                        # (B, nW, heads, 64, 64) fp32
        L = (s.astype(F64) * F64(F32(sc)) + b64[None, None].astype(F64)).astype(F32)                   # fmaf
        r64 = np.concatenate([reg, np.repeat(reg[:, NTOK - 1:], NPAD - NTOK, 1)], 1)                     # padded tokens: token 48's
        am = np.where(r64[:, :, None] != r64[:, None, :], F32(-100.0), F32(0.0)).astype(F32)
        L = L + am[None, :, None]
        pe = np.exp(L - L.max(-1, keepdims=True)).astype(F32)
        if defect == "no_half_exchange":
            half = (np.arange(NPAD) >> 2) & 1
            sums = np.stack([pe[..., half == h].sum(-1, dtype=F32) for h in (0, 1)], -1)
            inv = (F32(1) / sums)[..., (np.arange(DH) >> 2) & 1]
        else:
            inv = (F32(1) / pe.sum(-1, dtype=F32))[..., None]
        P = S.bf16_truncate(pe) if defect == "truncate_p" else S.bf(pe)
        vv = np.array(v)
        if defect == "v_key_order":
            vv[..., [32, 33], :] = vv[..., [33, 32], :]
        o = S.store((P @ vv).astype(F32) * inv, "bf16", mode)[..., :NTOK, :]      # (B, nW, heads, 49, 32)
        if defect == "window_pair_swap" and nwin == 2:
            o = o.reshape(B, nW // 2, 2, heads, NTOK, DH)[:, :, ::-1].reshape(B, nW, heads, NTOK, DH)
        orow = o.transpose(0, 1, 3, 2, 4).reshape(B * nW * NTOK, C)
        bp = np.array(op["bp"], F32)
        if defect == "drop_proj_bias":
            bp[32:64] = 0.0
        res = rows[idx0.reshape(-1)] if defect == "res_rolled" else xw
        if kernel == "swin_win96":
            y = G._gemm32(orow, op["wp"], acc=res) + bp
        else:
            y = (G._gemm32(orow, op["wp"]) + bp) + res
    out = np.full(rows.shape, SENTINEL, F32)
    out[idx0.reshape(-1) if defect == "roll_back_wrong" else flat] = y
    return out
