// Mixed-precision attention core for training on gfx950 (filter_value_and_grad(..., attn_dtype="bf16"); grad.py: g_qkv_attention):
// softmax(q k^T scale) v forward and backward on v_mfma_f32_32x32x16_bf16, fp32 in memory on both sides, N <= 256, dh 32 / 64.
// r(.) = fp32 -> bf16 round-to-nearest-even on the way into LDS / registers; everything else is fp32.
//
//   forward    s_ij = sum_d r(q_id) r(k_jd);  pe_ij = exp(scale (s_ij - max_j s_ij));  Z_i = sum_j pe_ij  (un-rounded pe)
//              out_i = (sum_j r(pe_ij) r(v_j)) / Z_i;  lse_i = scale max_j s_ij + log Z_i;  probs_ij = pe_ij / Z_i only when asked for
//   backward   p_ij = exp(scale s_ij - lse_i) recomputed;  delta_i = sum_d dout_id out_id (fp32, un-rounded)
//              dp_ij = sum_d r(dout_id) r(v_jd);  ds_ij = scale p_ij (dp_ij - delta_i)
//              dV_j = sum_i r(p_ij) r(dout_i);  dQ_i = sum_j r(ds_ij) r(k_j);  dK_j = sum_i r(ds_ij) r(q_i)
//
// LDS images, fragment readers and the row store: attn_mp_common.h (shared with swin_attn_mp.hip).
//
// Forward: one workgroup per (image, head), one wave per 32-query tile; the whole row of logits stays in the accumulators (attn.hip).
// Backward: one workgroup per (image, head) with Q, K, V, dO staged (a split over several, the pair re-staged, lost: amp_bwd_parts);
// the wave that owns a query tile walks the key tiles and accumulates dQ, then the wave that owns a key tile walks the query tiles,
// recomputes S, P and dS and accumulates dK and dV.  No atomics, one fixed summation order; dS never leaves the registers.
#include "attn_mp_common.h"

namespace mv {
namespace {

// ------------------------------------------------------------------------------------------------------------------ forward
template <int DH, int NT>
__global__ __launch_bounds__(512) void mha_mp_fwd_kernel(const float* __restrict__ qkv, float* __restrict__ out, float* __restrict__ lse,
                                                        float* __restrict__ probs, int N, int H, float scale) {
    constexpr int NP = NT * 32, PITCH = amp_pitch<DH>(), KC = DH / 16, DT = DH / 32;
    __shared__ __attribute__((aligned(16))) char smem[2 * NP * PITCH];
    char* kl = smem;
    char* vl = smem + NP * PITCH;

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, fr = lane & 31, fh = lane >> 5;
    const int pair = blockIdx.x, b = pair / H, h = pair - b * H;
    const long long rs = 3LL * H * DH;                                   // token-major [B, N, 3, H, dh]
    const float* qb = qkv + (long long)b * N * rs + (long long)h * DH;
    amp_stage<DH>(kl, N, NP, [&](int r) { return qb + (long long)H * DH + (long long)r * rs; });
    amp_stage<DH>(vl, N, NP, [&](int r) { return qb + 2LL * H * DH + (long long)r * rs; });

    // the wave's 32 queries, one per lane and half: r(q) straight into the B operand
    const int q = wave * 32 + fr;
    const bool qvalid = q < N;
    bf16x8 qf[KC];
    {
        const float* qp = qb + (long long)(qvalid ? q : N - 1) * rs + fh * 8;
#pragma unroll
        for (int kk = 0; kk < KC; ++kk) qf[kk] = amp_frag_mem(qp + kk * 16);
    }
    __syncthreads();

    // S^T = K . Q^T: register e of sacc[kt] = key 32 kt + (e & 3) + 8 (e >> 2) + 4 fh of the lane's query
    f32x16 sacc[NT];
#pragma unroll
    for (int kt = 0; kt < NT; ++kt) {
        amp_zero(sacc[kt]);
#pragma unroll
        for (int kk = 0; kk < KC; ++kk)
            sacc[kt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(amp_frag_c<DH>(kl, kt * 32, kk, lane), qf[kk], sacc[kt], 0, 0, 0);
    }
    float mx = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < NT; ++kt)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            float v = sacc[kt][e];
            if (kt == NT - 1) {                                          // only the last key tile holds padded keys
                const int key = kt * 32 + (e & 3) + 8 * (e >> 2) + 4 * fh;
                v = key < N ? v : -INFINITY;
                sacc[kt][e] = v;
            }
            mx = fmaxf(mx, v);
        }
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    // exp(scale (s - max)): the difference first, so that the winner's exponential is exactly 1 (a masked key: exp2(-inf) = 0)
    const float sl2 = scale * AMP_LOG2E;
    float sum = 0.f;
#pragma unroll
    for (int kt = 0; kt < NT; ++kt)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const float pe = __builtin_amdgcn_exp2f((sacc[kt][e] - mx) * sl2);
            sacc[kt][e] = pe;
            sum += pe;
        }
    sum += __shfl_xor(sum, 32);
    const float inv = 1.f / sum;
    const long long rowid = ((long long)b * H + h) * N + (qvalid ? q : 0);
    if (qvalid && fh == 0) lse[rowid] = scale * mx + logf(sum);
    if (probs && qvalid) {
        float* pr = probs + rowid * N;
#pragma unroll
        for (int kt = 0; kt < NT; ++kt)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int key = kt * 32 + (e & 3) + 8 * (e >> 2) + 4 * fh;
                if (kt < NT - 1 || key < N) pr[key] = sacc[kt][e] * inv;
            }
    }
    // O^T = V^T . P^T: step (kt, half) takes the keys of registers 8 half .. + 7 of sacc[kt], V read along its rows
    f32x16 oacc[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) amp_zero(oacc[dt]);
#pragma unroll
    for (int kt = 0; kt < NT; ++kt)
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            const bf16x8 pf = p_frag(sacc[kt], half);
#pragma unroll
            for (int dt = 0; dt < DT; ++dt)
                oacc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(amp_frag_t<DH>(vl, kt * 32 + 16 * half, dt * 32, lane), pf, oacc[dt], 0, 0, 0);
        }
    if (qvalid) amp_store_row<DT>(out + ((long long)b * N + q) * H * DH + (long long)h * DH, oacc, inv, fh);
}

// ------------------------------------------------------------------------------------------------------------------ backward
// One owner tile against every walked tile.  QOWN: the owner is 32 queries (one per lane), the walked rows are keys, the result dQ;
// else the owner is 32 keys, the walked rows are queries, the results dK (acc0) and dV (acc1).  Both products of a walked tile,
// S^T and dP^T [walked row][owner], have the walked rows in the registers: row 32 wt + (e & 3) + 8 (e >> 2) + 4 fh.
template <int DH, bool QOWN>
__device__ __forceinline__ void amp_bwd_walk(f32x16 (&acc0)[DH / 32], f32x16 (&acc1)[DH / 32], const char* ql, const char* kl, const char* vl,
                                             const char* gl, const float* lse_l, const float* del_l, int tile, int nt, int N, float scale,
                                             int lane) {
    constexpr int KC = DH / 16, DT = DH / 32;
    const int fr = lane & 31, fh = lane >> 5;
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
    const float lse_o = lse_l[tile * 32 + fr], del_o = del_l[tile * 32 + fr];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) { amp_zero(acc0[dt]); amp_zero(acc1[dt]); }

    for (int wt = 0; wt < nt; ++wt) {
        f32x16 s, dp;
        amp_zero(s);
        amp_zero(dp);
#pragma unroll
        for (int kk = 0; kk < KC; ++kk) {
            s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(amp_frag_c<DH>(wlk_s, wt * 32, kk, lane), bs[kk], s, 0, 0, 0);
            dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(amp_frag_c<DH>(wlk_p, wt * 32, kk, lane), bp[kk], dp, 0, 0, 0);
        }
        // p = exp(scale s - lse), ds = scale p (dp - delta); a padded key gets p = 0, a padded query has lse = +inf: p = 0
#pragma unroll
        for (int gq = 0; gq < 4; ++gq) {
            const int r0 = wt * 32 + 8 * gq + 4 * fh;                   // walked rows r0 .. r0 + 3 in registers 4 gq .. + 3
            float4 lw = make_float4(lse_o, lse_o, lse_o, lse_o), dw = make_float4(del_o, del_o, del_o, del_o);
            if (!QOWN) { lw = *(const float4*)(lse_l + r0); dw = *(const float4*)(del_l + r0); }
            const float ls[4] = {lw.x, lw.y, lw.z, lw.w}, dl[4] = {dw.x, dw.y, dw.z, dw.w};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int e = 4 * gq + i;
                float p = __builtin_amdgcn_exp2f((scale * s[e] - ls[i]) * AMP_LOG2E);
                if (QOWN && r0 + i >= N) p = 0.f;
                s[e] = p;
                dp[e] = scale * p * (dp[e] - dl[i]);
            }
        }
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            const bf16x8 dsf = p_frag(dp, half);
            const int row0 = wt * 32 + 16 * half;
            if (QOWN) {
#pragma unroll
                for (int dt = 0; dt < DT; ++dt)                          // dQ^T += K^T . dS^T
                    acc0[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(amp_frag_t<DH>(kl, row0, dt * 32, lane), dsf, acc0[dt], 0, 0, 0);
            } else {
                const bf16x8 pf = p_frag(s, half);
#pragma unroll
                for (int dt = 0; dt < DT; ++dt) {                        // dK^T += Q^T . dS,  dV^T += dO^T . P
                    acc0[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(amp_frag_t<DH>(ql, row0, dt * 32, lane), dsf, acc0[dt], 0, 0, 0);
                    acc1[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(amp_frag_t<DH>(gl, row0, dt * 32, lane), pf, acc1[dt], 0, 0, 0);
                }
            }
        }
    }
}

template <int DH>
__global__ __launch_bounds__(512) void mha_mp_bwd_kernel(const float* __restrict__ qkv, const float* __restrict__ out,
                                                        const float* __restrict__ dout, const float* __restrict__ lse,
                                                        float* __restrict__ dqkv, int N, int H, float scale) {
    constexpr int PITCH = amp_pitch<DH>(), DT = DH / 32;
    extern __shared__ __attribute__((aligned(16))) char amp_smem[];
    const int nt = (N + 31) / 32, NP = nt * 32;
    char* ql = amp_smem;
    char* kl = ql + NP * PITCH;
    char* vl = kl + NP * PITCH;
    char* gl = vl + NP * PITCH;
    float* lse_l = (float*)(gl + NP * PITCH);
    float* del_l = lse_l + NP;

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, fr = lane & 31, fh = lane >> 5;
    const int pair = blockIdx.x, b = pair / H, h = pair - b * H;
    const long long rs = 3LL * H * DH, os = (long long)H * DH;
    const float* qb = qkv + (long long)b * N * rs + (long long)h * DH;
    const float* ob = out + (long long)b * N * os + (long long)h * DH;
    const float* gb = dout + (long long)b * N * os + (long long)h * DH;
    amp_stage<DH>(ql, N, NP, [&](int r) { return qb + (long long)r * rs; });
    amp_stage<DH>(kl, N, NP, [&](int r) { return qb + os + (long long)r * rs; });
    amp_stage<DH>(vl, N, NP, [&](int r) { return qb + 2 * os + (long long)r * rs; });
    amp_stage<DH>(gl, N, NP, [&](int r) { return gb + (long long)r * os; });
    // delta_i = sum_d dout_id out_id in fp32 from the un-rounded operands: two threads per row, one half of dh each, in order
    for (int i = threadIdx.x; i < 2 * NP; i += blockDim.x) {
        const int row = i >> 1, hf = i & 1;
        float d = 0.f;
        if (row < N) {
            const float* op = ob + (long long)row * os + hf * (DH / 2);
            const float* gp = gb + (long long)row * os + hf * (DH / 2);
#pragma unroll
            for (int c = 0; c < DH / 8; ++c) {
                const float4 o4 = *(const float4*)(op + 4 * c), g4 = *(const float4*)(gp + 4 * c);
                d = fmaf(g4.x, o4.x, d); d = fmaf(g4.y, o4.y, d); d = fmaf(g4.z, o4.z, d); d = fmaf(g4.w, o4.w, d);
            }
        }
        d += __shfl_xor(d, 1);
        if (hf == 0) {
            del_l[row] = d;
            lse_l[row] = row < N ? lse[((long long)b * H + h) * N + row] : INFINITY;
        }
    }
    __syncthreads();

    // wave w owns tile blockIdx.y + gridDim.y w: as a query tile first, then as a key tile
    const int tile = blockIdx.y + gridDim.y * wave;
    if (tile >= nt) return;
    const int n = tile * 32 + fr;
    float* drow = dqkv + ((long long)b * N + (n < N ? n : 0)) * rs + (long long)h * DH;
    f32x16 a0[DT], a1[DT];
    amp_bwd_walk<DH, true>(a0, a1, ql, kl, vl, gl, lse_l, del_l, tile, nt, N, scale, lane);
    if (n < N) amp_store_row<DT>(drow, a0, 1.f, fh);
    amp_bwd_walk<DH, false>(a0, a1, ql, kl, vl, gl, lse_l, del_l, tile, nt, N, scale, lane);
    if (n < N) {
        amp_store_row<DT>(drow + os, a0, 1.f, fh);
        amp_store_row<DT>(drow + 2 * os, a1, 1.f, fh);
    }
}

size_t amp_bwd_lds(int N, int dh) {
    const size_t np = (size_t)((N + 31) / 32) * 32;
    return np * (4 * (size_t)(dh * 2 + 16) + 8);
}

// Workgroups per (image, head) in the backward, each staging the pair again and owning every parts-th tile.  Measured at N = 197,
// dh = 64, H = 12: one workgroup per pair wins at every batch -- 25 us against 26 / 36 / 65 us for 2 / 4 / 6 parts
// at B = 4 (48 pairs on 256 CUs), 124 us against 220 / 637 us at B = 64 -- so the product launches one; the split stays as a debug
// switch (tools/time_attn_mp.py --parts) that reproduces the measurement.
int amp_bwd_parts(int nt) {
    const int parts = get_flag("mha_mp_bwd_parts");
    return parts <= 0 ? 1 : parts > nt ? nt : parts;
}

template <int DH> int amp_fwd_launch(const float* qkv, float* out, float* lse, float* probs, int B, int N, int H, float scale, hipStream_t st) {
    const int nt = (N + 31) / 32;
    const dim3 grid((unsigned)(B * H)), block(64 * nt);
#define GO(NT_)                                                                                                            \
    case NT_:                                                                                                              \
        hipLaunchKernelGGL((mha_mp_fwd_kernel<DH, NT_>), grid, block, 0, st, qkv, out, lse, probs, N, H, scale);             \
        break;
    switch (nt) {
        GO(1) GO(2) GO(3) GO(4) GO(5) GO(6) GO(7) GO(8)
        default:
            set_error("mha_mp_fwd: N=%d unsupported", N);
            return MV_E_UNSUPPORTED;
    }
#undef GO
    MV_LAUNCH_CHECK();
    return MV_OK;
}

template <int DH> int amp_bwd_launch(const float* qkv, const float* out, const float* dout, const float* lse, float* dqkv, int B, int N, int H,
                                     float scale, hipStream_t st) {
    const int nt = (N + 31) / 32, parts = amp_bwd_parts(nt);
    const size_t smem = amp_bwd_lds(N, DH);
    auto kern = mha_mp_bwd_kernel<DH>;
    MV_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)amp_bwd_lds(256, DH)));
    hipLaunchKernelGGL(kern, dim3((unsigned)(B * H), (unsigned)parts), dim3(64 * ((nt + parts - 1) / parts)), smem, st, qkv, out, dout, lse,
                       dqkv, N, H, scale);
    MV_LAUNCH_CHECK();
    return MV_OK;
}

}  // namespace
}  // namespace mv

using namespace mv;

extern "C" {

int mv_mha_mp_supported(int N, int dh) { return (dh == 32 || dh == 64) && N >= 1 && N <= 256; }

int mv_mha_mp_fwd(const float* qkv, float* out, float* lse, float* probs, int B, int N, int H, int dh, float scale, mv_stream_t stream) {
    MV_CHECK_ARG(qkv && out && lse && B > 0 && H > 0 && scale > 0.f, "mha_mp_fwd: bad arguments");
    MV_CHECK_ARG(amp_aligned(qkv) && amp_aligned(out), "mha_mp_fwd: qkv / out must be 16-byte aligned");
    if (!mv_mha_mp_supported(N, dh) || (long long)B * H >= (1LL << 31)) {
        set_error("mha_mp_fwd: unsupported N=%d dh=%d B*H=%lld (dh 32 / 64, 1 <= N <= 256)", N, dh, (long long)B * H);
        return MV_E_UNSUPPORTED;
    }
    set_kernel_name(dh == 64 ? "mha_mp_fwd_dh64" : "mha_mp_fwd_dh32");
    if (dh == 64) return amp_fwd_launch<64>(qkv, out, lse, probs, B, N, H, scale, (hipStream_t)stream);
    return amp_fwd_launch<32>(qkv, out, lse, probs, B, N, H, scale, (hipStream_t)stream);
}

int mv_mha_mp_bwd(const float* qkv, const float* out, const float* dout, const float* lse, float* dqkv, int B, int N, int H, int dh,
                  float scale, mv_stream_t stream) {
    MV_CHECK_ARG(qkv && out && dout && lse && dqkv && B > 0 && H > 0 && scale > 0.f, "mha_mp_bwd: bad arguments");
    MV_CHECK_ARG(amp_aligned(qkv) && amp_aligned(out) && amp_aligned(dout) && amp_aligned(dqkv), "mha_mp_bwd: operands must be 16-byte aligned");
    if (!mv_mha_mp_supported(N, dh) || (long long)B * H >= (1LL << 31)) {
        set_error("mha_mp_bwd: unsupported N=%d dh=%d B*H=%lld (dh 32 / 64, 1 <= N <= 256)", N, dh, (long long)B * H);
        return MV_E_UNSUPPORTED;
    }
    set_kernel_name(dh == 64 ? "mha_mp_bwd_dh64" : "mha_mp_bwd_dh32");
    if (dh == 64) return amp_bwd_launch<64>(qkv, out, dout, lse, dqkv, B, N, H, scale, (hipStream_t)stream);
    return amp_bwd_launch<32>(qkv, out, dout, lse, dqkv, B, N, H, scale, (hipStream_t)stream);
}

}  // extern "C"
