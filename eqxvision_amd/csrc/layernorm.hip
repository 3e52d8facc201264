// The LayerNorm family: one wave (or part of one) per row, statistics in registers.  Plain / vectorised / slim LayerNorm, the
// post-norm residual step of Swin V2 and the patch-merge gather + LayerNorm, with their entries.
#include <type_traits>

#include "mfma_common.h"

namespace mv {

// LayerNorm: one wave per row, two-pass in registers/LDS-free (row re-read from L1/L2).
template <typename TI, typename TO>
__global__ void layernorm_kernel(const TI* __restrict__ x, const float* __restrict__ gamma,
                                 const float* __restrict__ beta, TO* __restrict__ y, long long M, int C,
                                 long long xs, float eps) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (row >= M) return;
    const TI* xr = x + row * xs;
    float s = 0.f;
    for (int c = lane; c < C; c += 64) s += io<TI>::ld(xr + c);
    const float mean = wave_sum(s) / (float)C;
    float v = 0.f;
    for (int c = lane; c < C; c += 64) {
        const float d = io<TI>::ld(xr + c) - mean;
        v += d * d;
    }
    const float rstd = rsqrtf(wave_sum(v) / (float)C + eps);
    TO* yr = y + row * C;
    for (int c = lane; c < C; c += 64) {
        float o = (io<TI>::ld(xr + c) - mean) * rstd;
        if (gamma) o *= gamma[c];
        if (beta) o += beta[c];
        io<TO>::st(yr + c, o);
    }
}

// Vectorised LayerNorm: one wave per row, the whole row held in registers, 16-byte loads.
// TI = bf16 (8 elements per 16-byte chunk) or fp32 (4 elements per chunk, the fp32 residual stream);
// TO = bf16 or fp32.  CHUNKS = 16-byte chunks per lane (row length <= 64 * CHUNKS chunks).
template <typename T> struct Vec16;
template <> struct Vec16<bf16_t> {
    static constexpr int N = 8;
    __device__ static __forceinline__ void ld(const bf16_t* p, float* v) {
        const uint4 u = *(const uint4*)p;
        const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            v[2 * e] = __uint_as_float(w[e] << 16);
            v[2 * e + 1] = __uint_as_float(w[e] & 0xffff0000u);
        }
    }
};
template <> struct Vec16<float> {
    static constexpr int N = 4;
    __device__ static __forceinline__ void ld(const float* p, float* v) {
        const float4 u = *(const float4*)p;
        v[0] = u.x; v[1] = u.y; v[2] = u.z; v[3] = u.w;
    }
};
template <typename TO, int N> struct StN;
template <> struct StN<bf16_t, 8> {
    __device__ static __forceinline__ void st(bf16_t* p, const float* o) {
        *(uint4*)p = make_uint4(pack_bf2(o[0], o[1]), pack_bf2(o[2], o[3]), pack_bf2(o[4], o[5]), pack_bf2(o[6], o[7]));
    }
};
template <> struct StN<bf16_t, 4> {
    __device__ static __forceinline__ void st(bf16_t* p, const float* o) {
        *(uint2*)p = make_uint2(pack_bf2(o[0], o[1]), pack_bf2(o[2], o[3]));
    }
};
template <> struct StN<float, 8> {
    __device__ static __forceinline__ void st(float* p, const float* o) {
        *(float4*)p = make_float4(o[0], o[1], o[2], o[3]);
        *(float4*)(p + 4) = make_float4(o[4], o[5], o[6], o[7]);
    }
};
template <> struct StN<float, 4> {
    __device__ static __forceinline__ void st(float* p, const float* o) { *(float4*)p = make_float4(o[0], o[1], o[2], o[3]); }
};

// WIDTH lanes cooperate on one row (64 / WIDTH rows per wave per step); every wave walks a grid-stride list of
// row groups and issues the NEXT group's loads before reducing the current one, so the row latency is hidden
// by the wave itself (the one-row-per-short-lived-wave version ran at 2.5 TB/s on [50432 x 768] fp32).
template <int WIDTH> __device__ __forceinline__ float group_sum(float v) {
#pragma unroll
    for (int o = WIDTH / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// The row code of the vectorised LayerNorms (layernorm_vec_kernel, layernorm_add_kernel): WIDTH lanes hold one row as CHUNKS chunks
// of N values each (chunk i of lane sl is live when sl + WIDTH * i < nch); two-pass mean / variance on the registers.
template <int N, int CHUNKS, int WIDTH>
__device__ __forceinline__ void row_stats(const float (*a)[N], int sl, int nch, float invC, float eps, float& mean, float& rstd) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < CHUNKS; ++i) {
        const bool on = sl + WIDTH * i < nch;
#pragma unroll
        for (int e = 0; e < N; ++e) s += on ? a[i][e] : 0.f;
    }
    mean = group_sum<WIDTH>(s) * invC;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < CHUNKS; ++i) {
        const bool on = sl + WIDTH * i < nch;
#pragma unroll
        for (int e = 0; e < N; ++e) {
            const float d = a[i][e] - mean;
            q += on ? d * d : 0.f;
        }
    }
    rstd = rsqrtf(group_sum<WIDTH>(q) * invC + eps);
}

template <typename TI, typename TO, int CHUNKS, int WIDTH>
__global__ __launch_bounds__(256) void layernorm_vec_kernel(const TI* __restrict__ x, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, TO* __restrict__ y, long long M,
                                                            int C, long long xs, float eps) {
    constexpr int N = Vec16<TI>::N;
    constexpr int RPW = 64 / WIDTH;                      // rows per wave per step
    const int lane = threadIdx.x & 63;
    const int sub = lane / WIDTH, sl = lane % WIDTH;     // which row of the group, lane within the row
    const long long gw = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const long long nw = (long long)gridDim.x * (blockDim.x >> 6);
    const int nch = C / N;
    const float invC = 1.0f / (float)C;

    // gamma / beta live in registers for the whole kernel (per-row re-loads through null checks were compiled
    // into 8 serialized scalar loads per chunk); chunk indices are clamped so every load is unconditional.
    float gm[CHUNKS][N], bt[CHUNKS][N];
    int cc[CHUNKS];
#pragma unroll
    for (int i = 0; i < CHUNKS; ++i) {
        const int c = sl + WIDTH * i;
        cc[i] = c < nch ? c : nch - 1;
#pragma unroll
        for (int e = 0; e < N; e += 4) {
            float4 gv = make_float4(1.f, 1.f, 1.f, 1.f), bv = make_float4(0.f, 0.f, 0.f, 0.f);
            if (gamma) gv = *(const float4*)(gamma + cc[i] * N + e);
            if (beta) bv = *(const float4*)(beta + cc[i] * N + e);
            gm[i][e] = gv.x; gm[i][e + 1] = gv.y; gm[i][e + 2] = gv.z; gm[i][e + 3] = gv.w;
            bt[i][e] = bv.x; bt[i][e + 1] = bv.y; bt[i][e + 2] = bv.z; bt[i][e + 3] = bv.w;
        }
    }

    float cur[CHUNKS][N], nxt[CHUNKS][N];
    const long long groups = (M + RPW - 1) / RPW;
    auto load = [&](float (*v)[N], long long group) {
        if (group >= groups) group = groups - 1;          // clamped re-read instead of a conditional load
        long long row = group * RPW + sub;
        if (row >= M) row = M - 1;
        const TI* xr = x + row * xs;
#pragma unroll
        for (int i = 0; i < CHUNKS; ++i) Vec16<TI>::ld(xr + cc[i] * N, v[i]);
    };
    // One step: issue the loads of the group after `gg` into `b`, then reduce / normalise / store `a`.  The
    // two register sets swap roles every step (loop unrolled by two) so nothing is copied and the wave only
    // ever waits for the OLDER of two row groups in flight.
    auto step = [&](float (*a)[N], float (*b)[N], long long gg) {
        load(b, gg + nw);
        asm volatile("" : "+v"(a[0][0]) : : "memory");  // keep the prefetch ahead of the arithmetic on `a`
        float mean, rstd;
        row_stats<N, CHUNKS, WIDTH>(a, sl, nch, invC, eps, mean, rstd);
        const long long row = gg * RPW + sub;
        const bool live = gg < groups && row < M;
        TO* yr = y + row * C;
#pragma unroll
        for (int i = 0; i < CHUNKS; ++i) {
            float o[N];
#pragma unroll
            for (int e = 0; e < N; ++e) o[e] = (a[i][e] - mean) * rstd * gm[i][e] + bt[i][e];
            if (live && sl + WIDTH * i < nch) StN<TO, N>::st(yr + cc[i] * N, o);
        }
    };
    long long g = gw;
    if (g >= groups) return;
    load(cur, g);
    for (; g < groups; g += 2 * nw) {
        step(cur, nxt, g);
        step(nxt, cur, g + nw);
    }
}

// Post-norm residual step (Swin V2: x + norm(branch(x)), swin.py:629-635; _PatchMergingV2's norm with res = NULL, :83-87):
//     y[m][:] = res[m][:] + gamma * n(z[m][:]) + beta      z bf16 / fp32, res fp32 or NULL, y fp32
// and, when y_lo is given, the same row rounded once to TL -- the operand plane the next Linear reads, so no cast launch stands in
// front of the GEMMs that consume the fp32 stream.  Row layout and statistics are layernorm_vec_kernel's (row_stats); one row group
// at a time per wave (the kernel is a plain stream: two reads, two writes).
template <typename TI, typename TL, int CHUNKS, int WIDTH>
__global__ __launch_bounds__(256) void layernorm_add_kernel(const TI* __restrict__ z, const float* __restrict__ res,
                                                            const float* __restrict__ gamma, const float* __restrict__ beta,
                                                            float* __restrict__ y, TL* __restrict__ y_lo, long long M, int C, float eps) {
    constexpr int N = Vec16<TI>::N;
    constexpr int RPW = 64 / WIDTH;
    const int lane = threadIdx.x & 63;
    const int sub = lane / WIDTH, sl = lane % WIDTH;
    const long long gw = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const long long nw = (long long)gridDim.x * (blockDim.x >> 6);
    const int nch = C / N;
    const float invC = 1.0f / (float)C;
    const long long groups = (M + RPW - 1) / RPW;
    int cc[CHUNKS];
#pragma unroll
    for (int i = 0; i < CHUNKS; ++i) {
        const int c = sl + WIDTH * i;
        cc[i] = c < nch ? c : nch - 1;
    }
    for (long long g = gw; g < groups; g += nw) {
        long long row = g * RPW + sub;
        const bool live = row < M;
        if (!live) row = M - 1;                           // clamped re-read: the group reductions need every lane
        float a[CHUNKS][N];
#pragma unroll
        for (int i = 0; i < CHUNKS; ++i) Vec16<TI>::ld(z + row * C + cc[i] * N, a[i]);
        float mean, rstd;
        row_stats<N, CHUNKS, WIDTH>(a, sl, nch, invC, eps, mean, rstd);
#pragma unroll
        for (int i = 0; i < CHUNKS; ++i) {
            if (!(live && sl + WIDTH * i < nch)) continue;
            const long long off = row * C + cc[i] * N;
            float o[N];
#pragma unroll
            for (int e = 0; e < N; e += 4) {
                const float4 gv = *(const float4*)(gamma + cc[i] * N + e), bv = *(const float4*)(beta + cc[i] * N + e);
                float4 rv = make_float4(0.f, 0.f, 0.f, 0.f);
                if (res) rv = *(const float4*)(res + off + e);
                o[e] = rv.x + ((a[i][e] - mean) * rstd * gv.x + bv.x);
                o[e + 1] = rv.y + ((a[i][e + 1] - mean) * rstd * gv.y + bv.y);
                o[e + 2] = rv.z + ((a[i][e + 2] - mean) * rstd * gv.z + bv.z);
                o[e + 3] = rv.w + ((a[i][e + 3] - mean) * rstd * gv.w + bv.w);
            }
            StN<float, N>::st(y + off, o);
            if (y_lo) StN<TL, N>::st(y_lo + off, o);
        }
    }
}

// The same LayerNorm on <= 64 VGPRs and no LDS (fp32 rows in, bf16 out, C = 256 * CHUNKS <= 1024): one wave per row, the row in
// CHUNKS x 4 registers, no second row in flight.  Alone it is slower than the kernel above; its point is WHERE it can run: a
// Linear-layer igemm8 workgroup (igemm8.hip, LIN) takes 8 waves x 224 VGPRs of a CU, which leaves 64 registers per SIMD lane --
// room for exactly one such wave per SIMD.  With two graph lanes the LayerNorm of one lane then runs UNDER the other lane's GEMM
// main loop (whose memory pipe is idle) instead of time-slicing the CUs with it.
template <int CHUNKS>
__global__ __launch_bounds__(256) void layernorm_slim_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                             const float* __restrict__ beta, bf16_t* __restrict__ y, long long M,
                                                             float eps) {
    constexpr int C = 256 * CHUNKS;
    const int lane = threadIdx.x & 63;
    const long long gw = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const long long nw = (long long)gridDim.x * 4;
    for (long long row = gw; row < M; row += nw) {
        const float* xr = x + row * C + lane * 4;
        float4 v[CHUNKS];
#pragma unroll
        for (int i = 0; i < CHUNKS; ++i) v[i] = *(const float4*)(xr + 256 * i);
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < CHUNKS; ++i) s += (v[i].x + v[i].y) + (v[i].z + v[i].w);
        const float mean = group_sum<64>(s) * (1.0f / C);
        float q = 0.f;
#pragma unroll
        for (int i = 0; i < CHUNKS; ++i) {
            v[i].x -= mean; v[i].y -= mean; v[i].z -= mean; v[i].w -= mean;
            q += (v[i].x * v[i].x + v[i].y * v[i].y) + (v[i].z * v[i].z + v[i].w * v[i].w);
        }
        const float rstd = rsqrtf(group_sum<64>(q) * (1.0f / C) + eps);
        bf16_t* yr = y + row * C + lane * 4;
#pragma unroll
        for (int i = 0; i < CHUNKS; ++i) {
            const float4 g = *(const float4*)(gamma + 256 * i + lane * 4), b = *(const float4*)(beta + 256 * i + lane * 4);
            *(uint2*)(yr + 256 * i) = make_uint2(pack_bf2(v[i].x * rstd * g.x + b.x, v[i].y * rstd * g.y + b.y),
                                                 pack_bf2(v[i].z * rstd * g.z + b.z, v[i].w * rstd * g.w + b.w));
        }
    }
}

// Swin patch merging (swin.py:23-31, 61-65): the 2 x 2 neighbourhood gather and the LayerNorm over its 4 C channels in ONE pass --
// a wave per output row reads the four C-float segments straight from the fp32 map ([x[0::2,0::2], x[1::2,0::2], x[0::2,1::2],
// x[1::2,1::2]] order), two-pass statistics in registers, bf16 (or fp32) rows out; the gathered 4C map is never materialised.
// NV = float4 per lane (4C / 256 rounded up); H, W even.
template <int NV, typename OutT>
__global__ __launch_bounds__(256) void patch_merge_ln_kernel(const float* __restrict__ x, const float* __restrict__ gam,
                                                             const float* __restrict__ bet, OutT* __restrict__ y, int B, int H, int W,
                                                             int C, float eps) {
    const int lane = threadIdx.x & 63;
    const int Ho = H / 2, Wo = W / 2, c4 = C / 4, q4 = 4 * c4;          // float4 per source pixel / per output row
    const long long rows = (long long)B * Ho * Wo;
    const long long w0 = (long long)blockIdx.x * 4 + (threadIdx.x >> 6), nw = (long long)gridDim.x * 4;
    float4 g[NV], bb[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int q = lane + 64 * i;
        g[i] = q < q4 ? ((const float4*)gam)[q] : make_float4(0, 0, 0, 0);
        bb[i] = q < q4 ? ((const float4*)bet)[q] : make_float4(0, 0, 0, 0);
    }
    for (long long m = w0; m < rows; m += nw) {
        const int wo = (int)(m % Wo);
        const long long t = m / Wo;
        const int ho = (int)(t % Ho), b = (int)(t / Ho);
        float4 v[NV];
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int q = lane + 64 * i;
            const int seg = q / c4, c = q - seg * c4;                  // segment 0..3 -> pixel (2 ho + (seg & 1), 2 wo + (seg >> 1))
            v[i] = make_float4(0, 0, 0, 0);
            if (q < q4) v[i] = ((const float4*)x)[(((long long)b * H + 2 * ho + (seg & 1)) * W + 2 * wo + (seg >> 1)) * c4 + c];
            s += (v[i].x + v[i].y) + (v[i].z + v[i].w);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
        const float mean = s / (float)(4 * C);
        float qq = 0.f;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            if (lane + 64 * i < q4) {
                v[i].x -= mean; v[i].y -= mean; v[i].z -= mean; v[i].w -= mean;
                qq += (v[i].x * v[i].x + v[i].y * v[i].y) + (v[i].z * v[i].z + v[i].w * v[i].w);
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) qq += __shfl_xor(qq, o);
        const float rstd = rsqrtf(qq / (float)(4 * C) + eps);
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int q = lane + 64 * i;
            if (q < q4) {
                const float4 o = make_float4(fmaf(v[i].x * rstd, g[i].x, bb[i].x), fmaf(v[i].y * rstd, g[i].y, bb[i].y),
                                             fmaf(v[i].z * rstd, g[i].z, bb[i].z), fmaf(v[i].w * rstd, g[i].w, bb[i].w));
                Out4<OutT>::st((void*)(y + m * 4 * C + 4 * q), o);
            }
        }
    }
}

// The launch shape of the vectorised LayerNorms (layernorm_vec_kernel, layernorm_add_kernel) for rows of nch 16-byte chunks:
// WIDTH lanes per row, CHUNKS chunks per lane, four waves per block; f(CHUNKS, WIDTH as integral constants, grid) launches.
template <class F> int ln_vec_launch(int nch, long long M, F&& f) {
    const int width = nch <= 16 ? 16 : (nch <= 32 ? 32 : 64);
    const int rpw = 64 / width;
    const long long groups = (M + rpw - 1) / rpw;
    long long nb = (groups + 3) / 4;
    if (nb > 256 * 8) nb = 256 * 8;
    const dim3 grid((unsigned)nb);
#define GO(CH, WD) return f(std::integral_constant<int, CH>{}, std::integral_constant<int, WD>{}, grid)
    if (width == 16) GO(1, 16);
    if (width == 32) GO(1, 32);
    if (nch <= 64) GO(1, 64);
    if (nch <= 128) GO(2, 64);
    if (nch <= 192) GO(3, 64);
    if (nch <= 256) GO(4, 64);
    if (nch <= 384) GO(6, 64);
    GO(8, 64);
#undef GO
}

}  // namespace mv

using namespace mv;

extern "C" {

int mv_layernorm_fwd(const void* x, const float* gamma, const float* beta, void* y, int64_t M, int C,
                     int64_t x_row_stride, float eps, int in_dtype, int out_dtype, mv_stream_t stream) {
    MV_CHECK_ARG(x && y && M > 0 && C > 0, "layernorm: bad args");
    const long long xs = x_row_stride ? (long long)x_row_stride : (long long)C;
    MV_CHECK_ARG(xs >= C, "layernorm: row stride %lld < C=%d", xs, C);
    hipStream_t st = (hipStream_t)stream;
    return dispatch_io("layernorm", in_dtype, out_dtype, [&](auto ti, auto to) -> int {
        using TI = decltype(ti); using TO = decltype(to);
        const int epc = Vec16<TI>::N;                         // elements per 16-byte chunk of the input
        const int nch = C / epc;
        if (!get_flag("no_ln_slim") && std::is_same<TI, float>::value && std::is_same<TO, bf16_t>::value && gamma && beta && xs == C &&
            C % 256 == 0 && C <= 768 && !get_flag("force_generic")) {
            set_kernel_name("layernorm_slim");
            long long nb = (M + 3) / 4;
            if (nb > 2048) nb = 2048;
            dim3 sgrid((unsigned)nb), sblock(256);
#define GOS(CH) hipLaunchKernelGGL((layernorm_slim_kernel<CH>), sgrid, sblock, 0, st, (const float*)x, gamma, beta, (bf16_t*)y, (long long)M, eps)
            if (C == 256) GOS(1);
            else if (C == 512) GOS(2);
            else if (C == 768) GOS(3);
            else GOS(4);
#undef GOS
            MV_LAUNCH_CHECK();
            return MV_OK;
        }
        if (C % epc == 0 && xs % epc == 0 && nch <= 64 * 8 && !get_flag("force_generic")) {
            set_kernel_name("layernorm_vec");
            return ln_vec_launch(nch, M, [&](auto ch, auto wd, dim3 vgrid) -> int {
                hipLaunchKernelGGL((layernorm_vec_kernel<TI, TO, decltype(ch)::value, decltype(wd)::value>), vgrid, dim3(256), 0, st,
                                   (const TI*)x, gamma, beta, (TO*)y, (long long)M, C, xs, eps);
                MV_LAUNCH_CHECK();
                return MV_OK;
            });
        }
        set_kernel_name("layernorm");
        const int rows_per_block = 4;
        dim3 grid((unsigned)((M + rows_per_block - 1) / rows_per_block)), block(64 * rows_per_block);
        hipLaunchKernelGGL((layernorm_kernel<TI, TO>), grid, block, 0, st, (const TI*)x, gamma, beta, (TO*)y, (long long)M, C, xs, eps);
        MV_LAUNCH_CHECK();
        return MV_OK;
    });
}

int mv_layernorm_add_fwd(const void* z, const float* res, const float* gamma, const float* beta, float* y, void* y_lo, int64_t M,
                         int C, float eps, int z_dtype, int lo_dtype, mv_stream_t stream) {
    MV_CHECK_ARG(z && gamma && beta && y && M > 0 && C > 0, "layernorm_add: bad args");
    MV_CHECK_ARG((const void*)y != z && y_lo != z, "layernorm_add: an output aliases z");
    hipStream_t st = (hipStream_t)stream;
    return dispatch_io("layernorm_add", z_dtype, lo_dtype, [&](auto ti, auto tl) -> int {
        using TI = decltype(ti); using TL = decltype(tl);
        const int epc = Vec16<TI>::N;
        const int nch = C / epc;
        if (C % epc || nch > 64 * 8) {
            set_error("layernorm_add: unsupported width C=%d (whole 16-byte chunks of z, at most 512 of them)", C);
            return MV_E_UNSUPPORTED;
        }
        set_kernel_name("layernorm_add");
        return ln_vec_launch(nch, M, [&](auto ch, auto wd, dim3 vgrid) -> int {
            hipLaunchKernelGGL((layernorm_add_kernel<TI, TL, decltype(ch)::value, decltype(wd)::value>), vgrid, dim3(256), 0, st,
                               (const TI*)z, res, gamma, beta, y, (TL*)y_lo, (long long)M, C, eps);
            MV_LAUNCH_CHECK();
            return MV_OK;
        });
    });
}

int mv_patch_merge_ln_supported(int H, int W, int C, int x_dtype) {
    return !get_flag("no_patch_merge_ln") && x_dtype == MV_F32 && H % 2 == 0 && W % 2 == 0 && C % 4 == 0 && C <= 384 && C >= 16;
}

int mv_patch_merge_ln_fwd(const void* x, const float* gamma, const float* beta, void* y, int B, int H, int W, int C, float eps,
                          int x_dtype, int out_dtype, mv_stream_t stream) {
    MV_CHECK_ARG(x && gamma && beta && y && B > 0, "patch_merge_ln: bad args");
    if (!mv_patch_merge_ln_supported(H, W, C, x_dtype)) {
        set_error("mv_patch_merge_ln_fwd: unsupported %dx%dx%d (ask mv_patch_merge_ln_supported first)", H, W, C);
        return MV_E_UNSUPPORTED;
    }
    hipStream_t st = (hipStream_t)stream;
    const long long rows = (long long)B * (H / 2) * (W / 2);
    long long blocks = (rows + 3) / 4;
    if (blocks > 256 * 8) blocks = 256 * 8;
    const int nv = (C + 63) / 64;                       // float4 per lane: 4C / 4 / 64
    set_kernel_name("patch_merge_ln_f32in");
    return dispatch_dtype("patch_merge_ln", out_dtype, [&](auto to) -> int {
        using TO = decltype(to);
#define MV_PML(NVV)                                                                                                                 \
    hipLaunchKernelGGL((patch_merge_ln_kernel<NVV, TO>), dim3((unsigned)blocks), dim3(256), 0, st, (const float*)x, gamma, beta, (TO*)y, \
                       B, H, W, C, eps)
        if (nv <= 2) MV_PML(2);
        else if (nv <= 3) MV_PML(3);
        else MV_PML(6);
#undef MV_PML
        MV_LAUNCH_CHECK();
        return MV_OK;
    });
}

}  // extern "C"
