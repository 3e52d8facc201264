// ConvNeXt block head: the 7x7 depthwise convolution and the channel LayerNorm that follows it, in one pass, NHWC, gfx950
// (reference convnext.py:16-72: `Conv2d(dim, dim, 7, padding=3, groups=dim)` -> `LayerNorm2d(dim)`).
//
//   d[b,h,w,c] = bias[c] + sum_{r,s<7} x[b, h+r-3, w+s-3, c] * w[r][s][c]          (zero padding, fp32 accumulation)
//   normalize = 0:  y = d                                    (the consumer normalises: mv_ln_mlp_res_fwd / mv_ln_mlp_stream_res_fwd)
//   normalize = 1:  y = (d - mean_c d) * rsqrt(var_c d + eps)   (biased var; the LayerNorm affine is folded into fc1 by the caller)
//
// One workgroup owns TW consecutive output pixels of one image row and ALL C channels (what the statistics need); TW is sized by C
// so that the tile stays a few KB to 80 KB of LDS (TW = 32 at C = 96 ... 4 at C >= 768).  The seven input rows of the window pass
// through LDS one at a time as fp32 ((TW + 6) x C values, the row's seven filter vectors next to them as bf16): every input element
// is fetched by 7 x (1 + 6 / TW) workgroups, not by the 49 taps of each of its outputs (the generic depthwise kernel does two
// unshared 16-byte loads per tap).  A thread owns 8 consecutive channels of one pixel per item (up to 3 items), reads its taps from
// LDS and keeps its accumulators in registers across the rows.  With normalize = 1 the d tile is parked in the (dead) row buffer,
// one wave per pixel takes the row statistics in TWO passes over the kept values (mean, then the mean of squared deviations:
// rows with a large common offset lose nothing to cancellation), and the normalised values leave as bf16.
#include "mfma_common.h"

namespace mv {

namespace {

constexpr int CNB_THREADS = 256, CNB_KI = 3, CNB_K = 7;

struct CnbP {
    const void* x;
    const bf16_t* w;      // [7][7][C]
    const float* bias;    // [C] or null
    void* y;
    int N, H, W, C, TW;
    float eps;
};

template <typename XT> struct CnbIn;
template <> struct CnbIn<float> {
    __device__ static __forceinline__ void ld8(const float* p, float4& a, float4& b) {
        a = *(const float4*)p;
        b = *(const float4*)(p + 4);
    }
};
template <> struct CnbIn<bf16_t> {
    __device__ static __forceinline__ void ld8(const bf16_t* p, float4& a, float4& b) {
        const uint4 u = *(const uint4*)p;
        a = make_float4(__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xffff0000u), __uint_as_float(u.y << 16),
                        __uint_as_float(u.y & 0xffff0000u));
        b = make_float4(__uint_as_float(u.z << 16), __uint_as_float(u.z & 0xffff0000u), __uint_as_float(u.w << 16),
                        __uint_as_float(u.w & 0xffff0000u));
    }
};

int cnb_tile(int C) {
    int tw = 32;
    while (tw > 4 && tw * C > 4096) tw >>= 1;
    return tw;
}

size_t cnb_smem(int C, int TW) { return (size_t)(TW + CNB_K - 1) * C * 4 + (size_t)CNB_K * C * 2 + (size_t)TW * 8; }

template <typename XT, typename YT, bool NORM>
__global__ __launch_bounds__(CNB_THREADS) void cnblock_dw_kernel(const CnbP p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int C = p.C, G = C >> 3, TW = p.TW, XW = TW + CNB_K - 1;
    float* xs = (float*)smem;                                     // [XW][C] one input row of the window (later: the d tile)
    bf16_t* ws = (bf16_t*)(xs + (size_t)XW * C);                  // [7][C] the row's filter vectors
    float* stat = (float*)(ws + CNB_K * C);                       // [TW][2] mean, rstd
    const int tid = threadIdx.x;
    const int w0 = blockIdx.x * TW, h = blockIdx.y, b = blockIdx.z;
    const XT* x = (const XT*)p.x;
    const long long img = (long long)b * p.H;

    const int items = TW * G;
    int ip[CNB_KI], ic[CNB_KI];
    float acc[CNB_KI][8];
#pragma unroll
    for (int k = 0; k < CNB_KI; ++k) {
        const int it = tid + k * CNB_THREADS;
        ip[k] = it < items ? it / G : -1;
        ic[k] = it < items ? (it - ip[k] * G) * 8 : 0;
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[k][e] = 0.f;
    }

    for (int r = 0; r < CNB_K; ++r) {
        const int hi = h + r - CNB_K / 2;
        if (hi < 0 || hi >= p.H) continue;                        // uniform over the workgroup
        const XT* xrow = x + ((img + hi) * p.W) * C;
        for (int i = tid; i < XW * G; i += CNB_THREADS) {
            const int col = i / G, c = (i - col * G) * 8, wi = w0 - CNB_K / 2 + col;
            float4 a = make_float4(0.f, 0.f, 0.f, 0.f), bb = a;
            if (wi >= 0 && wi < p.W) CnbIn<XT>::ld8(xrow + (long long)wi * C + c, a, bb);
            *(float4*)(xs + col * C + c) = a;
            *(float4*)(xs + col * C + c + 4) = bb;
        }
        for (int i = tid; i < CNB_K * G; i += CNB_THREADS)
            *(uint4*)(ws + i * 8) = *(const uint4*)(p.w + (size_t)r * CNB_K * C + (size_t)i * 8);
        __syncthreads();
#pragma unroll
        for (int k = 0; k < CNB_KI; ++k) {
            if (ip[k] < 0) continue;
            const float* xp = xs + ip[k] * C + ic[k];
            const bf16_t* wp = ws + ic[k];
#pragma unroll
            for (int s = 0; s < CNB_K; ++s) {
                const float4 a = *(const float4*)(xp + s * C), bb = *(const float4*)(xp + s * C + 4);
                const uint4 u = *(const uint4*)(wp + s * C);
                acc[k][0] = fmaf(a.x, __uint_as_float(u.x << 16), acc[k][0]);
                acc[k][1] = fmaf(a.y, __uint_as_float(u.x & 0xffff0000u), acc[k][1]);
                acc[k][2] = fmaf(a.z, __uint_as_float(u.y << 16), acc[k][2]);
                acc[k][3] = fmaf(a.w, __uint_as_float(u.y & 0xffff0000u), acc[k][3]);
                acc[k][4] = fmaf(bb.x, __uint_as_float(u.z << 16), acc[k][4]);
                acc[k][5] = fmaf(bb.y, __uint_as_float(u.z & 0xffff0000u), acc[k][5]);
                acc[k][6] = fmaf(bb.z, __uint_as_float(u.w << 16), acc[k][6]);
                acc[k][7] = fmaf(bb.w, __uint_as_float(u.w & 0xffff0000u), acc[k][7]);
            }
        }
        __syncthreads();
    }

#pragma unroll
    for (int k = 0; k < CNB_KI; ++k) {
        if (ip[k] < 0 || !p.bias) continue;
        const float4 a = *(const float4*)(p.bias + ic[k]), bb = *(const float4*)(p.bias + ic[k] + 4);
        acc[k][0] += a.x; acc[k][1] += a.y; acc[k][2] += a.z; acc[k][3] += a.w;
        acc[k][4] += bb.x; acc[k][5] += bb.y; acc[k][6] += bb.z; acc[k][7] += bb.w;
    }

    if (NORM) {
        // park d, then one wave per pixel: two passes over the kept values
#pragma unroll
        for (int k = 0; k < CNB_KI; ++k) {
            if (ip[k] < 0) continue;
            float* dp = xs + ip[k] * C + ic[k];
            *(float4*)dp = make_float4(acc[k][0], acc[k][1], acc[k][2], acc[k][3]);
            *(float4*)(dp + 4) = make_float4(acc[k][4], acc[k][5], acc[k][6], acc[k][7]);
        }
        __syncthreads();
        const int lane = tid & 63, wave = tid >> 6;
        const float inv = 1.0f / (float)C;
        for (int px = wave; px < TW; px += CNB_THREADS / 64) {
            const float* dr = xs + px * C;
            float s = 0.f;
            for (int c = lane; c < C; c += 64) s += dr[c];
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o);
            const float mean = s * inv;
            float q = 0.f;
            for (int c = lane; c < C; c += 64) {
                const float dv = dr[c] - mean;
                q = fmaf(dv, dv, q);
            }
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) q += __shfl_xor(q, o);
            if (lane == 0) {
                stat[2 * px] = mean;
                stat[2 * px + 1] = rsqrtf(q * inv + p.eps);
            }
        }
        __syncthreads();
    }

#pragma unroll
    for (int k = 0; k < CNB_KI; ++k) {
        if (ip[k] < 0 || w0 + ip[k] >= p.W) continue;
        float o[8];
        if (NORM) {
            const float mean = stat[2 * ip[k]], rstd = stat[2 * ip[k] + 1];
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = (acc[k][e] - mean) * rstd;
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = acc[k][e];
        }
        Out8<YT>::st((YT*)p.y + ((img + h) * p.W + w0 + ip[k]) * C + ic[k], o);
    }
}

template <typename XT, typename YT, bool NORM>
int cnb_go(const CnbP& p, hipStream_t st) {
    static LdsAttrSite site;
    auto kern = cnblock_dw_kernel<XT, YT, NORM>;
    const size_t smem = cnb_smem(p.C, p.TW);
    MV_HIP(site.ensure((const void*)kern, smem));
    hipLaunchKernelGGL(kern, dim3((unsigned)((p.W + p.TW - 1) / p.TW), (unsigned)p.H, (unsigned)p.N), dim3(CNB_THREADS), smem, st, p);
    MV_LAUNCH_CHECK();
    return MV_OK;
}

}  // namespace

}  // namespace mv

extern "C" {

int mv_cnblock_dw_supported(int C, int H, int W, int x_dtype, int y_dtype, int normalize) {
    if (mv::get_flag("no_cnblock_dw") || mv::get_flag("force_generic")) return 0;
    if (C < 8 || C > 1536 || C % 8 || H < 1 || W < 1 || H > 65535) return 0;
    if (x_dtype != MV_F32 && x_dtype != MV_BF16) return 0;
    if (normalize) return normalize == 1 && y_dtype == MV_BF16;
    return y_dtype == MV_BF16 || y_dtype == MV_F32;
}

int mv_cnblock_dw_fwd(const void* x, const void* w_rsc, const float* bias, void* y, int N, int H, int W, int C, float eps,
                      int normalize, int x_dtype, int y_dtype, mv_stream_t stream_) {
    using namespace mv;
    MV_CHECK_ARG(x && w_rsc && y, "mv_cnblock_dw_fwd: null argument");
    MV_CHECK_ARG(x != y, "mv_cnblock_dw_fwd: not in place");
    MV_CHECK_ARG(N >= 1 && N <= 65535, "mv_cnblock_dw_fwd: N=%d", N);
    if (!mv_cnblock_dw_supported(C, H, W, x_dtype, y_dtype, normalize)) {
        set_error("mv_cnblock_dw_fwd: unsupported C=%d H=%d W=%d x_dtype=%d y_dtype=%d normalize=%d (ask mv_cnblock_dw_supported first)",
                  C, H, W, x_dtype, y_dtype, normalize);
        return MV_E_UNSUPPORTED;
    }
    CnbP p;
    p.x = x; p.w = (const bf16_t*)w_rsc; p.bias = bias; p.y = y;
    p.N = N; p.H = H; p.W = W; p.C = C; p.TW = cnb_tile(C); p.eps = eps;
    hipStream_t st = (hipStream_t)stream_;
    const bool xf = x_dtype == MV_F32;
    if (normalize) {
        set_kernel_name(xf ? "cnblock_dw7_ln_f32in" : "cnblock_dw7_ln_bf16in");
        return xf ? cnb_go<float, bf16_t, true>(p, st) : cnb_go<bf16_t, bf16_t, true>(p, st);
    }
    if (y_dtype == MV_F32) {
        set_kernel_name(xf ? "cnblock_dw7_f32in_f32out" : "cnblock_dw7_bf16in_f32out");
        return xf ? cnb_go<float, float, false>(p, st) : cnb_go<bf16_t, float, false>(p, st);
    }
    set_kernel_name(xf ? "cnblock_dw7_f32in" : "cnblock_dw7_bf16in");
    return xf ? cnb_go<float, bf16_t, false>(p, st) : cnb_go<bf16_t, bf16_t, false>(p, st);
}

}  // extern "C"
