// Pooling over NHWC maps: max pool, adaptive and global average pool (memory-bound VALU kernels) and their entries.
#include <type_traits>

#include "mfma_common.h"

namespace mv {

template <typename T>
__global__ void maxpool_nhwc_kernel(const T* __restrict__ x, T* __restrict__ y, int N, int H, int W, int C, int Ho,
                                    int Wo, int kh, int kw, int sh, int sw, int ph, int pw) {
    const long long total = (long long)N * Ho * Wo * C;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        long long m = i / C;
        const int wo = (int)(m % Wo);
        m /= Wo;
        const int ho = (int)(m % Ho);
        const int n = (int)(m / Ho);
        float best = -INFINITY;
        for (int r = 0; r < kh; ++r) {
            const int hi = ho * sh - ph + r;
            if (hi < 0 || hi >= H) continue;
            for (int s = 0; s < kw; ++s) {
                const int wi = wo * sw - pw + s;
                if (wi < 0 || wi >= W) continue;
                best = fmaxf(best, io<T>::ld(x + (((long long)n * H + hi) * W + wi) * C + c));
            }
        }
        io<T>::st(y + i, best);
    }
}

// 8 bf16 channels per thread (16-byte loads/stores), C % 8 == 0
__global__ void maxpool_nhwc_bf16x8_kernel(const uint4* __restrict__ x, uint4* __restrict__ y, int N, int H, int W,
                                           int C8, int Ho, int Wo, int kh, int kw, int sh, int sw, int ph, int pw) {
    const long long total = (long long)N * Ho * Wo * C8;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(i % C8);
        long long m = i / C8;
        const int wo = (int)(m % Wo);
        m /= Wo;
        const int ho = (int)(m % Ho);
        const int n = (int)(m / Ho);
        float best[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) best[e] = -INFINITY;
        for (int r = 0; r < kh; ++r) {
            const int hi = ho * sh - ph + r;
            if (hi < 0 || hi >= H) continue;
            for (int s = 0; s < kw; ++s) {
                const int wi = wo * sw - pw + s;
                if (wi < 0 || wi >= W) continue;
                const uint4 v = x[(((long long)n * H + hi) * W + wi) * C8 + c];
                const uint32_t u[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    best[2 * e] = fmaxf(best[2 * e], __uint_as_float(u[e] << 16));
                    best[2 * e + 1] = fmaxf(best[2 * e + 1], __uint_as_float(u[e] & 0xffff0000u));
                }
            }
        }
        uint4 o;
        // inputs are exact bf16 values, max is exact: truncation == rounding
        o.x = (__float_as_uint(best[0]) >> 16) | (__float_as_uint(best[1]) & 0xffff0000u);
        o.y = (__float_as_uint(best[2]) >> 16) | (__float_as_uint(best[3]) & 0xffff0000u);
        o.z = (__float_as_uint(best[4]) >> 16) | (__float_as_uint(best[5]) & 0xffff0000u);
        o.w = (__float_as_uint(best[6]) >> 16) | (__float_as_uint(best[7]) & 0xffff0000u);
        y[i] = o;
    }
}

__device__ __forceinline__ void adaptive_bounds(int n, int t, int i, int& lo, int& hi) {
    // equinox AdaptiveAvgPool rule
    if (n % t == 0) {
        const int k = n / t;
        lo = i * k;
        hi = lo + k;
    } else {
        const int big = n % t, k = n / t;
        if (i < big) {
            lo = i * (k + 1);
            hi = lo + k + 1;
        } else {
            lo = big * (k + 1) + (i - big) * k;
            hi = lo + k;
        }
    }
}

template <typename TI, typename TO>
__global__ void adaptive_avgpool_nhwc_kernel(const TI* __restrict__ x, TO* __restrict__ y, int N, int H, int W,
                                             int C, int oh, int ow) {
    const long long total = (long long)N * oh * ow * C;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        long long m = i / C;
        const int j = (int)(m % ow);
        m /= ow;
        const int ii = (int)(m % oh);
        const int n = (int)(m / oh);
        int h0, h1, w0, w1;
        adaptive_bounds(H, oh, ii, h0, h1);
        adaptive_bounds(W, ow, j, w0, w1);
        float s = 0.f;
        for (int hh = h0; hh < h1; ++hh)
            for (int ww = w0; ww < w1; ++ww) s += io<TI>::ld(x + (((long long)n * H + hh) * W + ww) * C + c);
        io<TO>::st(y + i, s / (float)((h1 - h0) * (w1 - w0)));
    }
}

// Global average pool (oh = ow = 1) of a bf16 NHWC map, 8 channels (16 bytes) per thread, pixels unrolled 4-wide
// so several loads are in flight (the element-per-thread kernel above is latency-bound: 10 us for 12.8 MB).
template <typename TO>
__global__ void global_avgpool_bf16x8_kernel(const uint4* __restrict__ x, TO* __restrict__ y, int N, int HW, int C8) {
    const long long total = (long long)N * C8;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (long long)gridDim.x * blockDim.x) {
        const int c8 = (int)(i % C8);
        const int n = (int)(i / C8);
        const uint4* xp = x + (long long)n * HW * C8 + c8;
        float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        int p = 0;
        for (; p + 4 <= HW; p += 4) {
            uint4 v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = xp[(long long)(p + j) * C8];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t w[4] = {v[j].x, v[j].y, v[j].z, v[j].w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    s[2 * e] += __uint_as_float(w[e] << 16);
                    s[2 * e + 1] += __uint_as_float(w[e] & 0xffff0000u);
                }
            }
        }
        for (; p < HW; ++p) {
            const uint4 v = xp[(long long)p * C8];
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                s[2 * e] += __uint_as_float(w[e] << 16);
                s[2 * e + 1] += __uint_as_float(w[e] & 0xffff0000u);
            }
        }
        const float inv = 1.f / (float)HW;
#pragma unroll
        for (int e = 0; e < 8; ++e) io<TO>::st(y + i * 8 + e, s[e] * inv);
    }
}

// The same reduction for LARGE maps (squeeze-excitation on 112 x 112 ... 14 x 14 maps, layers/squeeze.py:56; DeepLab's pooled
// branch): one thread per (image, 8 channels) would walk 12 544 pixels serially with a few thousand threads on the whole chip
// (measured 1.27 ms for 128 x 112 x 112 x 32).  Here a block of 256 threads owns one image and up to 32 channel chunks; the
// threads of a chunk stride over the pixels (whole 128-byte lines per pixel across the chunk lanes) and meet in LDS.
template <typename TI, typename TO>
__global__ __launch_bounds__(1024) void global_avgpool_wide_kernel(const TI* __restrict__ x, TO* __restrict__ y, int HW, int C8,
                                                                   int cpb, int pl) {
    __shared__ float red[1024 * 8];
    const int n = blockIdx.x, c8 = blockIdx.y * cpb + (int)threadIdx.x % cpb, lp = (int)threadIdx.x / cpb;
    const long long C = (long long)C8 * 8;
    float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (lp < pl && c8 < C8) {
        const TI* xp = x + (long long)n * HW * C + c8 * 8;
        auto ld = [&](int p, float4& a, float4& b) {
            a = Out4<TI>::ld(xp + (long long)p * C);
            b = Out4<TI>::ld(xp + (long long)p * C + 4);
        };
        auto acc = [&](const float4& a, const float4& b) {
            s[0] += a.x; s[1] += a.y; s[2] += a.z; s[3] += a.w; s[4] += b.x; s[5] += b.y; s[6] += b.z; s[7] += b.w;
        };
        int p = lp;
        for (; p + 3 * pl < HW; p += 4 * pl) {              // four pixels in flight per thread (1024 threads per image: the block
            float4 a[4], b[4];                              // count is only images x channel chunks)
#pragma unroll
            for (int u = 0; u < 4; ++u) ld(p + u * pl, a[u], b[u]);
#pragma unroll
            for (int u = 0; u < 4; ++u) acc(a[u], b[u]);
        }
        for (; p < HW; p += pl) {
            float4 a, b;
            ld(p, a, b);
            acc(a, b);
        }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) red[threadIdx.x * 8 + e] = s[e];
    __syncthreads();
    if (lp == 0 && c8 < C8) {
        for (int q = 1; q < pl; ++q)
#pragma unroll
            for (int e = 0; e < 8; ++e) s[e] += red[(q * cpb + (int)threadIdx.x) * 8 + e];
        const float inv = 1.f / (float)HW;
#pragma unroll
        for (int e = 0; e < 8; ++e) io<TO>::st(y + ((long long)n * C8 + c8) * 8 + e, s[e] * inv);
    }
}

}  // namespace mv

using namespace mv;

extern "C" {

int mv_maxpool2d_nhwc_fwd(const void* x, void* y, int N, int H, int W, int C, int kh, int kw, int sh, int sw, int ph,
                          int pw, int dtype, mv_stream_t stream) {
    MV_CHECK_ARG(x && y && N > 0 && H > 0 && W > 0 && C > 0 && kh > 0 && kw > 0 && sh > 0 && sw > 0, "maxpool: bad args");
    MV_CHECK_ARG(2 * ph <= kh && 2 * pw <= kw, "maxpool: padding larger than half the window");
    const int Ho = (H + 2 * ph - kh) / sh + 1, Wo = (W + 2 * pw - kw) / sw + 1;
    MV_CHECK_ARG(Ho > 0 && Wo > 0, "maxpool: empty output");
    hipStream_t st = (hipStream_t)stream;
    return dispatch_dtype("maxpool", dtype, [&](auto t) -> int {
        using T = decltype(t);
        if (std::is_same<T, bf16_t>::value && C % 8 == 0) {
            set_kernel_name("maxpool_nhwc_bf16x8");
            const long long total = (long long)N * Ho * Wo * (C / 8);
            hipLaunchKernelGGL(maxpool_nhwc_bf16x8_kernel, dim3(grid_for(total)), dim3(256), 0, st, (const uint4*)x,
                               (uint4*)y, N, H, W, C / 8, Ho, Wo, kh, kw, sh, sw, ph, pw);
        } else {
            set_kernel_name("maxpool_nhwc");
            const long long total = (long long)N * Ho * Wo * C;
            hipLaunchKernelGGL(maxpool_nhwc_kernel<T>, dim3(grid_for(total)), dim3(256), 0, st, (const T*)x, (T*)y, N, H, W, C, Ho,
                               Wo, kh, kw, sh, sw, ph, pw);
        }
        MV_LAUNCH_CHECK();
        return MV_OK;
    });
}

int mv_adaptive_avgpool2d_nhwc_fwd(const void* x, void* y, int N, int H, int W, int C, int oh, int ow, int in_dtype,
                                   int out_dtype, mv_stream_t stream) {
    MV_CHECK_ARG(x && y && N > 0 && H > 0 && W > 0 && C > 0 && oh > 0 && ow > 0 && oh <= H && ow <= W, "avgpool: bad args");
    hipStream_t st = (hipStream_t)stream;
    const long long total = (long long)N * oh * ow * C;
    return dispatch_io("avgpool", in_dtype, out_dtype, [&](auto ti, auto to) -> int {
        using TI = decltype(ti); using TO = decltype(to);
        constexpr bool in_bf16 = std::is_same<TI, bf16_t>::value;
        if (oh == 1 && ow == 1 && C % 8 == 0 && !get_flag("force_generic")) {
            // a block per (image, 32-channel-vector chunk): big maps always; small maps too when one thread per (image, 8 channels)
            // would leave most of the chip without a wave (squeeze-excitation on 14 x 14 / 7 x 7 maps at 128 images; Swin's last map in fp32)
            const bool wide = (long long)H * W >= 256 || ((long long)H * W >= 32 && (long long)N * (C / 8) <= 24576);
            if (wide && N <= 65535) {
                const int C8 = C / 8, cpb = C8 < 32 ? C8 : 32, pl = 1024 / cpb;
                set_kernel_name(in_bf16 ? "global_avgpool_wide_bf16x8" : "global_avgpool_wide_f32x8");
                dim3 g((unsigned)N, (unsigned)((C8 + cpb - 1) / cpb));
                hipLaunchKernelGGL((global_avgpool_wide_kernel<TI, TO>), g, dim3(1024), 0, st, (const TI*)x, (TO*)y, H * W, C8, cpb, pl);
                MV_LAUNCH_CHECK();
                return MV_OK;
            }
            if constexpr (in_bf16) {
                set_kernel_name("global_avgpool_bf16x8");
                const long long nt = (long long)N * (C / 8);
                hipLaunchKernelGGL(global_avgpool_bf16x8_kernel<TO>, dim3(grid_for(nt, 64)), dim3(64), 0, st, (const uint4*)x, (TO*)y, N,
                                   H * W, C / 8);
                MV_LAUNCH_CHECK();
                return MV_OK;
            }
        }
        set_kernel_name("adaptive_avgpool_nhwc");
        hipLaunchKernelGGL((adaptive_avgpool_nhwc_kernel<TI, TO>), dim3(grid_for(total)), dim3(256), 0, st, (const TI*)x, (TO*)y, N, H,
                           W, C, oh, ow);
        MV_LAUNCH_CHECK();
        return MV_OK;
    });
}

}  // extern "C"
