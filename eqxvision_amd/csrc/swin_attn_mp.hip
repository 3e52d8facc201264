// Mixed-precision Swin shifted-window attention for training on gfx950 (filter_value_and_grad(..., attn_dtype="bf16"); grad.py:
// g_swin_window_attention): forward and backward on v_mfma_f32_32x32x16_bf16, fp32 in memory on both sides, windows of n <= 64 tokens
// (padded to two 32-row tiles), dh 32 / 64.  r(.) = fp32 -> bf16 round-to-nearest-even on the way into LDS / registers; everything
// else is fp32.
//
//   forward    l_ij = scale sum_d r(q_id) r(k_jd) + bias[h][i][j] + (shifted and region_i != region_j ? -100 : 0); keys j >= n: -inf
//              pe_ij = exp(l_ij - max_j l_ij);  Z_i = sum_j pe_ij (un-rounded);  out_i = (sum_j r(pe_ij) r(v_j)) / Z_i
//              lse_i = max_j l_ij + log Z_i
//   backward   p_ij = exp(l_ij - lse_i) recomputed;  delta_i = sum_d dout_id out_id (fp32, un-rounded)
//              dp_ij = sum_d r(dout_id) r(v_jd);  g_ij = p_ij (dp_ij - delta_i)
//              dV_j = sum_i r(p_ij) r(dout_i);  dQ_i = scale sum_j r(g_ij) r(k_j);  dK_j = scale sum_i r(g_ij) r(q_i)
//              dbias[h][i][j] = sum over images and windows of the un-rounded g_ij
// q is rounded as it is in memory: the scale multiplies the fp32 product (the fp32 kernels scale q first).
//
// Mapping, both kernels: a workgroup of two waves serves ONE head and walks the (image, window) pairs part, part + P, part + 2 P, ..
// (P = swa_parts: at most SWA_MAX_WGS workgroups in all, whatever the batch).  Wave w owns the window's 32-token tile w: as a query
// tile in the forward; in the backward as a query tile first (dQ, and g for the bias gradient), then as a key tile (dK, dV) with S, P
// and g recomputed, as in attn_mp.hip.  Rows are gathered and scattered through swin_tok_row; nothing rolled or partitioned is ever
// written.
//   * forward: the head's bias rows sit in the registers for the whole walk, in the order of the accumulator they are added to
//     (swin_attn_core.h: register e of s[kt] = key 32 kt + (e & 3) + 8 (e >> 2) + 4 fh of the lane's query).
//   * backward: the head's bias tile is staged once per workgroup as an fp32 [64][68] LDS tile (zero outside n x n) and read in the
//     register order of either orientation -- a float4 per register quad when the wave owns queries, four rows of one column when it
//     owns keys.  (Two register copies next to the dbias accumulators would not leave the dh = 64 walk its registers.)
//   * bias gradient: each wave adds the g of its 32 queries x 64 keys into 32 fp32 registers in walk order.  The two waves own
//     disjoint query rows, so there is nothing to combine between them; the workgroup writes part [part][head][n][n] once, at the end
//     of its walk -- all of it, zeros if it walked nothing.  No atomics; the parts are summed by the caller (mv_colsum_f32).
#include "attn_mp_common.h"
#include "swin_geom.h"

namespace mv {
namespace {

constexpr int SWA_NP = 64;              // a window's tokens, padded: two 32-row tiles
constexpr int SWA_BP = 68;              // fp32 pitch of the backward's bias tile
#ifndef MV_SWA_MAX_WGS                  // a build-time constant (P stays a function of the entry's arguments alone); other values
#define MV_SWA_MAX_WGS 2048             // were built with -DMV_SWA_MAX_WGS=.. and timed: DESIGN.md 3.3
#endif
constexpr int SWA_MAX_WGS = MV_SWA_MAX_WGS;   // workgroups of a launch, at most: 8 per CU of an MI355X

struct SwaP {
    WindowGeom g;
    int C, heads, n, nWw, nW;
    long long pairs;                    // B * nW
    float scale;
};

int swa_parts(long long pairs, int heads) {
    const long long cap = SWA_MAX_WGS / heads > 0 ? SWA_MAX_WGS / heads : 1;
    return (int)(pairs < cap ? (pairs < 1 ? 1 : pairs) : cap);
}

__device__ __forceinline__ int swa_key(int kt, int e, int fh) { return 32 * kt + (e & 3) + 8 * (e >> 2) + 4 * fh; }

// ------------------------------------------------------------------------------------------------------------------ forward
template <int DH>
__global__ __launch_bounds__(128) void swin_attn_mp_fwd_kernel(const float* __restrict__ qkv, const float* __restrict__ bias,
                                                              float* __restrict__ out, float* __restrict__ lse, SwaP P) {
    constexpr int PITCH = amp_pitch<DH>(), KC = DH / 16, DT = DH / 32;
    __shared__ __attribute__((aligned(16))) char smem[2 * SWA_NP * PITCH];
    __shared__ __attribute__((aligned(16))) int reg_l[SWA_NP];
    char* kl = smem;
    char* vl = smem + SWA_NP * PITCH;

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, fr = lane & 31, fh = lane >> 5;
    const int h = blockIdx.y, n = P.n, C = P.C;
    const int q = wave * 32 + fr;
    const bool qvalid = q < n, active = wave * 32 < n, shifted = P.g.shh + P.g.shw > 0;

    // the lane's query row of the head's bias, in accumulator order; 0 where there is no query or no key
    float bq[2][16];
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int key = swa_key(kt, e, fh);
            bq[kt][e] = (qvalid && key < n) ? bias[((long long)h * n + q) * n + key] : 0.f;
        }

    for (long long t = blockIdx.x; t < P.pairs; t += gridDim.x) {
        const int b = (int)(t / P.nW), win = (int)(t - (long long)b * P.nW), wy = win / P.nWw, wx = win - wy * P.nWw;
        const float* kb = qkv + C + (long long)h * DH;
        amp_stage<DH>(kl, n, SWA_NP, [&](int r) { return kb + swin_tok_row(P.g, b, wy, wx, r) * 3 * C; });
        amp_stage<DH>(vl, n, SWA_NP, [&](int r) { return kb + C + swin_tok_row(P.g, b, wy, wx, r) * 3 * C; });
        if (threadIdx.x < SWA_NP) reg_l[threadIdx.x] = (shifted && (int)threadIdx.x < n) ? swin_tok_region(P.g, wy, wx, threadIdx.x) : 0;
        const long long qrow = swin_tok_row(P.g, b, wy, wx, qvalid ? q : 0);
        bf16x8 qf[KC];
#pragma unroll
        for (int kk = 0; kk < KC; ++kk) qf[kk] = amp_frag_mem(qkv + qrow * 3 * C + (long long)h * DH + fh * 8 + kk * 16);
        __syncthreads();

        if (active) {
            // S^T = K . Q^T: register e of sacc[kt] = key swa_key(kt, e, fh) of the lane's query
            f32x16 sacc[2];
#pragma unroll
            for (int kt = 0; kt < 2; ++kt) {
                amp_zero(sacc[kt]);
#pragma unroll
                for (int kk = 0; kk < KC; ++kk)
                    sacc[kt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(amp_frag_c<DH>(kl, kt * 32, kk, lane), qf[kk], sacc[kt], 0, 0, 0);
            }
            const int qreg = reg_l[qvalid ? q : 0];
            float mx = -INFINITY;
#pragma unroll
            for (int kt = 0; kt < 2; ++kt)
#pragma unroll
                for (int gq = 0; gq < 4; ++gq) {
                    const int key0 = 32 * kt + 8 * gq + 4 * fh;
                    const int4 kr = *(const int4*)(reg_l + key0);
                    const int rr[4] = {kr.x, kr.y, kr.z, kr.w};
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int e = 4 * gq + i;
                        const float v = win_logit(sacc[kt][e], P.scale, bq[kt][e], shifted && rr[i] != qreg, key0 + i >= n);
                        sacc[kt][e] = v;
                        mx = fmaxf(mx, v);
                    }
                }
            mx = fmaxf(mx, __shfl_xor(mx, 32));
            float sum = 0.f;
#pragma unroll
            for (int kt = 0; kt < 2; ++kt)
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const float pe = __builtin_amdgcn_exp2f((sacc[kt][e] - mx) * AMP_LOG2E);   // the winner: exactly 1
                    sacc[kt][e] = pe;
                    sum += pe;
                }
            sum += __shfl_xor(sum, 32);
            const float inv = 1.f / sum;
            if (qvalid && fh == 0) lse[(t * P.heads + h) * n + q] = mx + logf(sum);
            // O^T = V^T . P^T: step (kt, half) takes the keys of registers 8 half .. + 7 of sacc[kt], V read along its rows
            f32x16 oacc[DT];
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) amp_zero(oacc[dt]);
#pragma unroll
            for (int kt = 0; kt < 2; ++kt)
#pragma unroll
                for (int half = 0; half < 2; ++half) {
                    const bf16x8 pf = p_frag(sacc[kt], half);
#pragma unroll
                    for (int dt = 0; dt < DT; ++dt)
                        oacc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(amp_frag_t<DH>(vl, kt * 32 + 16 * half, dt * 32, lane), pf, oacc[dt], 0, 0, 0);
                }
            if (qvalid) amp_store_row<DT>(out + qrow * C + (long long)h * DH, oacc, inv, fh);
        }
        __syncthreads();                                                     // the next pair overwrites the images
    }
}

// ------------------------------------------------------------------------------------------------------------------ backward
// One owner tile against the window's two walked tiles (attn_mp.hip: amp_bwd_walk, with the bias, the mask and the bias gradient).
// QOWN: the owner is 32 queries (one per lane), the walked rows are keys, the result dQ (acc0) and, if DB, gacc[wt] += g; else the
// owner is 32 keys, the walked rows are queries, the results dK (acc0) and dV (acc1).  Both products of a walked tile have the walked
// rows in the registers: row 32 wt + (e & 3) + 8 (e >> 2) + 4 fh.  The scale of dQ / dK is left to the store.
template <int DH, bool QOWN, bool DB>
__device__ __forceinline__ void swa_bwd_walk(f32x16 (&acc0)[DH / 32], f32x16 (&acc1)[DH / 32], f32x16 (&gacc)[2], const char* ql,
                                             const char* kl, const char* vl, const char* gl, const float* bias_l, const int* reg_l,
                                             const float* lse_l, const float* del_l, int tile, int n, float scale, bool shifted, int lane) {
    constexpr int KC = DH / 16, DT = DH / 32;
    const int fr = lane & 31, fh = lane >> 5, own = tile * 32 + fr;
    const char* own_s = QOWN ? ql : kl;          // the owner's operand of S      (walked: the other of q / k)
    const char* own_p = QOWN ? gl : vl;          // the owner's operand of dP     (walked: the other of dO / v)
    const char* wlk_s = QOWN ? kl : ql;
    const char* wlk_p = QOWN ? vl : gl;
    bf16x8 bs[KC], bp[KC];
#pragma unroll
    for (int kk = 0; kk < KC; ++kk) {
        bs[kk] = amp_frag_c<DH>(own_s, tile * 32, kk, lane);
        bp[kk] = amp_frag_c<DH>(own_p, tile * 32, kk, lane);
    }
    const float lse_o = lse_l[own], del_o = del_l[own];
    const int reg_o = reg_l[own];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) { amp_zero(acc0[dt]); amp_zero(acc1[dt]); }

#pragma unroll
    for (int wt = 0; wt < 2; ++wt) {
        f32x16 s, dp;
        amp_zero(s);
        amp_zero(dp);
#pragma unroll
        for (int kk = 0; kk < KC; ++kk) {
            s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(amp_frag_c<DH>(wlk_s, wt * 32, kk, lane), bs[kk], s, 0, 0, 0);
            dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(amp_frag_c<DH>(wlk_p, wt * 32, kk, lane), bp[kk], dp, 0, 0, 0);
        }
        // l = scale s + bias + mask, p = exp(l - lse), g = p (dp - delta); a padded key gets p = 0, a padded query has lse = +inf: p = 0
#pragma unroll
        for (int gq = 0; gq < 4; ++gq) {
            const int r0 = wt * 32 + 8 * gq + 4 * fh;                   // walked rows r0 .. r0 + 3 in registers 4 gq .. + 3
            float4 lw = make_float4(lse_o, lse_o, lse_o, lse_o), dw = make_float4(del_o, del_o, del_o, del_o), bw;
            if (QOWN) {
                bw = *(const float4*)(bias_l + own * SWA_BP + r0);      // bias[query own][keys r0 ..]
            } else {
                lw = *(const float4*)(lse_l + r0);
                dw = *(const float4*)(del_l + r0);
                bw = make_float4(bias_l[r0 * SWA_BP + own], bias_l[(r0 + 1) * SWA_BP + own], bias_l[(r0 + 2) * SWA_BP + own],
                                 bias_l[(r0 + 3) * SWA_BP + own]);     // bias[queries r0 ..][key own]
            }
            const int4 kr = *(const int4*)(reg_l + r0);
            const float ls[4] = {lw.x, lw.y, lw.z, lw.w}, dl[4] = {dw.x, dw.y, dw.z, dw.w}, bb[4] = {bw.x, bw.y, bw.z, bw.w};
            const int rr[4] = {kr.x, kr.y, kr.z, kr.w};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int e = 4 * gq + i;
                const float l = win_logit(s[e], scale, bb[i], shifted && rr[i] != reg_o, QOWN && r0 + i >= n);
                const float p = __builtin_amdgcn_exp2f((l - ls[i]) * AMP_LOG2E);           // a padded key: exp2(-inf) = 0
                const float g = p * (dp[e] - dl[i]);
                s[e] = p;
                dp[e] = g;
                if (QOWN && DB) gacc[wt][e] += g;
            }
        }
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            const bf16x8 gf = p_frag(dp, half);
            const int row0 = wt * 32 + 16 * half;
            if (QOWN) {
#pragma unroll
                for (int dt = 0; dt < DT; ++dt)                          // dQ^T += K^T . g^T
                    acc0[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(amp_frag_t<DH>(kl, row0, dt * 32, lane), gf, acc0[dt], 0, 0, 0);
            } else {
                const bf16x8 pf = p_frag(s, half);
#pragma unroll
                for (int dt = 0; dt < DT; ++dt) {                        // dK^T += Q^T . g,  dV^T += dO^T . P
                    acc0[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(amp_frag_t<DH>(ql, row0, dt * 32, lane), gf, acc0[dt], 0, 0, 0);
                    acc1[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(amp_frag_t<DH>(gl, row0, dt * 32, lane), pf, acc1[dt], 0, 0, 0);
                }
            }
        }
    }
}

template <int DH, bool DB>
__global__ __launch_bounds__(128, 2) void swin_attn_mp_bwd_kernel(const float* __restrict__ qkv, const float* __restrict__ bias,
                                                              const float* __restrict__ out, const float* __restrict__ dout,
                                                              const float* __restrict__ lse, float* __restrict__ dqkv,
                                                              float* __restrict__ dbias_parts, SwaP P) {
    constexpr int PITCH = amp_pitch<DH>(), DT = DH / 32;
    __shared__ __attribute__((aligned(16))) char smem[4 * SWA_NP * PITCH];
    __shared__ __attribute__((aligned(16))) float bias_l[SWA_NP * SWA_BP];
    __shared__ __attribute__((aligned(16))) float lse_l[SWA_NP];
    __shared__ __attribute__((aligned(16))) float del_l[SWA_NP];
    __shared__ __attribute__((aligned(16))) int reg_l[SWA_NP];
    __shared__ long long row_l[SWA_NP];
    char* ql = smem;
    char* kl = ql + SWA_NP * PITCH;
    char* vl = kl + SWA_NP * PITCH;
    char* gl = vl + SWA_NP * PITCH;

    const int lane = threadIdx.x & 63, tile = threadIdx.x >> 6, fr = lane & 31, fh = lane >> 5;
    const int h = blockIdx.y, n = P.n, C = P.C;
    const bool active = tile * 32 < n, shifted = P.g.shh + P.g.shw > 0;
    const int tok = tile * 32 + fr;

    for (int i = threadIdx.x; i < SWA_NP * SWA_NP; i += blockDim.x) {
        const int r = i >> 6, c = i & 63;
        bias_l[r * SWA_BP + c] = (r < n && c < n) ? bias[((long long)h * n + r) * n + c] : 0.f;
    }
    f32x16 gacc[2];
    amp_zero(gacc[0]);
    amp_zero(gacc[1]);

    for (long long t = blockIdx.x; t < P.pairs; t += gridDim.x) {
        const int b = (int)(t / P.nW), win = (int)(t - (long long)b * P.nW), wy = win / P.nWw, wx = win - wy * P.nWw;
        if (threadIdx.x < SWA_NP) {
            const int r = threadIdx.x;
            row_l[r] = r < n ? swin_tok_row(P.g, b, wy, wx, r) : 0;
            reg_l[r] = (shifted && r < n) ? swin_tok_region(P.g, wy, wx, r) : 0;
        }
        __syncthreads();
        const float* qb = qkv + (long long)h * DH;
        const float* ob = out + (long long)h * DH;
        const float* gb = dout + (long long)h * DH;
        amp_stage<DH>(ql, n, SWA_NP, [&](int r) { return qb + row_l[r] * 3 * C; });
        amp_stage<DH>(kl, n, SWA_NP, [&](int r) { return qb + C + row_l[r] * 3 * C; });
        amp_stage<DH>(vl, n, SWA_NP, [&](int r) { return qb + 2 * C + row_l[r] * 3 * C; });
        amp_stage<DH>(gl, n, SWA_NP, [&](int r) { return gb + row_l[r] * C; });
        // delta_i = sum_d dout_id out_id in fp32 from the un-rounded operands: two threads per row, one half of dh each, in order
        {
            const int row = threadIdx.x >> 1, hf = threadIdx.x & 1;
            float d = 0.f;
            if (row < n) {
                const float* op = ob + row_l[row] * C + hf * (DH / 2);
                const float* gp = gb + row_l[row] * C + hf * (DH / 2);
#pragma unroll
                for (int c = 0; c < DH / 8; ++c) {
                    const float4 o4 = *(const float4*)(op + 4 * c), g4 = *(const float4*)(gp + 4 * c);
                    d = fmaf(g4.x, o4.x, d); d = fmaf(g4.y, o4.y, d); d = fmaf(g4.z, o4.z, d); d = fmaf(g4.w, o4.w, d);
                }
            }
            d += __shfl_xor(d, 1);
            if (hf == 0) {
                del_l[row] = d;
                lse_l[row] = row < n ? lse[(t * P.heads + h) * n + row] : INFINITY;
            }
        }
        __syncthreads();

        if (active) {
            float* drow = dqkv + row_l[tok < n ? tok : 0] * 3 * C + (long long)h * DH;
            f32x16 a0[DT], a1[DT];
            swa_bwd_walk<DH, true, DB>(a0, a1, gacc, ql, kl, vl, gl, bias_l, reg_l, lse_l, del_l, tile, n, P.scale, shifted, lane);
            if (tok < n) amp_store_row<DT>(drow, a0, P.scale, fh);
            swa_bwd_walk<DH, false, DB>(a0, a1, gacc, ql, kl, vl, gl, bias_l, reg_l, lse_l, del_l, tile, n, P.scale, shifted, lane);
            if (tok < n) {
                amp_store_row<DT>(drow + C, a0, P.scale, fh);
                amp_store_row<DT>(drow + 2 * C, a1, 1.f, fh);
            }
        }
        __syncthreads();                                                     // the next pair overwrites the images and the tables
    }

    if (DB && tok < n) {                                                     // the workgroup's part: every element, once
        float* part = dbias_parts + (((long long)blockIdx.x * P.heads + h) * n + tok) * n;
#pragma unroll
        for (int wt = 0; wt < 2; ++wt)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int key = swa_key(wt, e, fh);
                if (key < n) part[key] = gacc[wt][e];
            }
    }
}

// the shared argument check: geometry, support, grid; fills P and the number of parts
int swa_check(const char* who, int B, int Hf, int Wf, int C, int heads, int ws_h, int ws_w, int shift_h, int shift_w, float scale, SwaP& P,
              int& parts) {
    MV_CHECK_ARG(B > 0 && Hf > 0 && Wf > 0 && C > 0 && heads > 0 && heads <= 65535 && scale > 0.f, "%s: bad arguments", who);
    const int rc = swin_check_geom(who, Hf, Wf, C, heads, ws_h, ws_w, shift_h, shift_w, P.g);
    if (rc != MV_OK) return rc;
    const long long n = (long long)ws_h * ws_w, nW = (long long)(Hf / ws_h) * (Wf / ws_w), pairs = (long long)B * nW;
    const int dh = C / heads;
    if (!(n <= 64 && mv_swin_attn_mp_supported((int)n, dh)) || pairs * heads >= (1LL << 31)) {
        set_error("%s: unsupported window of %lld tokens, dh=%d, B*nW*heads=%lld (dh 32 / 64, 1 <= n <= 64)", who, n, dh, pairs * heads);
        return MV_E_UNSUPPORTED;
    }
    P.C = C; P.heads = heads; P.n = (int)n; P.nWw = Wf / ws_w; P.nW = (int)nW; P.pairs = pairs; P.scale = scale;
    parts = swa_parts(pairs, heads);
    return MV_OK;
}

}  // namespace
}  // namespace mv

using namespace mv;

extern "C" {

int mv_swin_attn_mp_supported(int n_tokens, int dh) { return (dh == 32 || dh == 64) && n_tokens >= 1 && n_tokens <= 64; }

int mv_swin_attn_mp_bwd_parts(int B, int Hf, int Wf, int heads, int ws_h, int ws_w) {
    if (B <= 0 || Hf <= 0 || Wf <= 0 || heads <= 0 || ws_h <= 0 || ws_w <= 0) return 1;
    return swa_parts((long long)B * (Hf / ws_h) * (Wf / ws_w), heads);
}

int mv_swin_attn_mp_fwd(const float* qkv, const float* bias, float* out, float* lse, int B, int Hf, int Wf, int C, int heads, int ws_h,
                        int ws_w, int shift_h, int shift_w, float scale, mv_stream_t stream) {
    MV_CHECK_ARG(qkv && bias && out && lse, "swin_attn_mp_fwd: bad arguments");
    MV_CHECK_ARG(amp_aligned(qkv) && amp_aligned(bias) && amp_aligned(out) && amp_aligned(lse), "swin_attn_mp_fwd: operands must be 16-byte aligned");
    SwaP P;
    int parts;
    const int rc = swa_check("swin_attn_mp_fwd", B, Hf, Wf, C, heads, ws_h, ws_w, shift_h, shift_w, scale, P, parts);
    if (rc != MV_OK) return rc;
    const dim3 grid((unsigned)parts, (unsigned)heads), block(128);
    if (C / heads == 64) {
        set_kernel_name("swin_attn_mp_fwd_dh64");
        hipLaunchKernelGGL(swin_attn_mp_fwd_kernel<64>, grid, block, 0, (hipStream_t)stream, qkv, bias, out, lse, P);
    } else {
        set_kernel_name("swin_attn_mp_fwd_dh32");
        hipLaunchKernelGGL(swin_attn_mp_fwd_kernel<32>, grid, block, 0, (hipStream_t)stream, qkv, bias, out, lse, P);
    }
    MV_LAUNCH_CHECK();
    return MV_OK;
}

int mv_swin_attn_mp_bwd(const float* qkv, const float* bias, const float* out, const float* dout, const float* lse, float* dqkv,
                        float* dbias_parts, int B, int Hf, int Wf, int C, int heads, int ws_h, int ws_w, int shift_h, int shift_w,
                        float scale, mv_stream_t stream) {
    MV_CHECK_ARG(qkv && bias && out && dout && lse && dqkv, "swin_attn_mp_bwd: bad arguments");
    MV_CHECK_ARG(amp_aligned(qkv) && amp_aligned(bias) && amp_aligned(out) && amp_aligned(dout) && amp_aligned(lse) && amp_aligned(dqkv) &&
                     amp_aligned(dbias_parts),
                 "swin_attn_mp_bwd: operands must be 16-byte aligned");
    SwaP P;
    int parts;
    const int rc = swa_check("swin_attn_mp_bwd", B, Hf, Wf, C, heads, ws_h, ws_w, shift_h, shift_w, scale, P, parts);
    if (rc != MV_OK) return rc;
    const dim3 grid((unsigned)parts, (unsigned)heads), block(128);
    const hipStream_t st = (hipStream_t)stream;
    const bool d64 = C / heads == 64;
    if (dbias_parts) {
        set_kernel_name(d64 ? "swin_attn_mp_bwd_dh64_dbias" : "swin_attn_mp_bwd_dh32_dbias");
        if (d64) hipLaunchKernelGGL((swin_attn_mp_bwd_kernel<64, true>), grid, block, 0, st, qkv, bias, out, dout, lse, dqkv, dbias_parts, P);
        else hipLaunchKernelGGL((swin_attn_mp_bwd_kernel<32, true>), grid, block, 0, st, qkv, bias, out, dout, lse, dqkv, dbias_parts, P);
    } else {
        set_kernel_name(d64 ? "swin_attn_mp_bwd_dh64" : "swin_attn_mp_bwd_dh32");
        if (d64) hipLaunchKernelGGL((swin_attn_mp_bwd_kernel<64, false>), grid, block, 0, st, qkv, bias, out, dout, lse, dqkv, dbias_parts, P);
        else hipLaunchKernelGGL((swin_attn_mp_bwd_kernel<32, false>), grid, block, 0, st, qkv, bias, out, dout, lse, dqkv, dbias_parts, P);
    }
    MV_LAUNCH_CHECK();
    return MV_OK;
}

}  // extern "C"
