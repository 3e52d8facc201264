// eqx.nn.MaxPool2d(use_ceil=True) (reference squeezenet.py:88-112): max pooling with the output size given by the caller.  The ceil
// size is the floor size + 1 wherever (size + 2 pad - kernel) % stride != 0 (equinox pads the right / bottom by `stride` more); the
// taps of that last window that fall outside the map are skipped, like the taps of the ordinary padding.  NHWC, bf16 / fp32; the
// maximum of exact values is exact.
#include "common.h"

namespace mv {

namespace {

template <typename T>
__global__ __launch_bounds__(256) void maxpool_out_kernel(const T* __restrict__ x, T* __restrict__ y, int N, int H, int W, int C, int Ho,
                                                          int Wo, int kh, int kw, int sh, int sw, int ph, int pw) {
    const long long total = (long long)N * Ho * Wo * C;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
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

// 8 bf16 channels per thread (16-byte loads / stores), C % 8 == 0
__global__ __launch_bounds__(256) void maxpool_out_bf16x8_kernel(const uint4* __restrict__ x, uint4* __restrict__ y, int N, int H, int W,
                                                                 int C8, int Ho, int Wo, int kh, int kw, int sh, int sw, int ph, int pw) {
    const long long total = (long long)N * Ho * Wo * C8;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
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
        uint4 o;                                                     // exact bf16 values in, exact maximum out: truncation == rounding
        o.x = (__float_as_uint(best[0]) >> 16) | (__float_as_uint(best[1]) & 0xffff0000u);
        o.y = (__float_as_uint(best[2]) >> 16) | (__float_as_uint(best[3]) & 0xffff0000u);
        o.z = (__float_as_uint(best[4]) >> 16) | (__float_as_uint(best[5]) & 0xffff0000u);
        o.w = (__float_as_uint(best[6]) >> 16) | (__float_as_uint(best[7]) & 0xffff0000u);
        y[i] = o;
    }
}

unsigned pool_grid(long long total) {
    long long g = (total + 255) / 256;
    return (unsigned)(g > 256 * 32 ? 256 * 32 : g);
}

// true when `out` is the floor or the ceil output size of one axis and its last window still holds a tap of the map
bool pool_axis_ok(int size, int k, int s, int p, int out) {
    const int span = size + 2 * p - k;
    if (span < 0) return false;
    const int lo = span / s + 1, hi = lo + (span % s != 0 ? 1 : 0);
    if (out != lo && out != hi) return false;
    return (out - 1) * s - p < size;
}

}  // namespace

}  // namespace mv

extern "C" {

int mv_maxpool2d_out_nhwc_fwd(const void* x, void* y, int N, int H, int W, int C, int kh, int kw, int sh, int sw, int ph, int pw, int Ho,
                              int Wo, int dtype, mv_stream_t stream) {
    using namespace mv;
    MV_CHECK_ARG(x && y && N > 0 && H > 0 && W > 0 && C > 0 && kh > 0 && kw > 0 && sh > 0 && sw > 0 && ph >= 0 && pw >= 0,
                 "maxpool_out: bad args");
    MV_CHECK_ARG(dtype == MV_F32 || dtype == MV_BF16, "maxpool_out: dtype %d", dtype);
    MV_CHECK_ARG(2 * ph <= kh && 2 * pw <= kw, "maxpool_out: padding larger than half the window");
    MV_CHECK_ARG(pool_axis_ok(H, kh, sh, ph, Ho) && pool_axis_ok(W, kw, sw, pw, Wo),
                 "maxpool_out: output %d x %d is neither the floor nor the ceil size of %d x %d (window %d x %d, stride %d x %d, padding "
                 "%d x %d), or its last window lies outside the map", Ho, Wo, H, W, kh, kw, sh, sw, ph, pw);
    hipStream_t st = (hipStream_t)stream;
    if (dtype == MV_BF16 && C % 8 == 0) {
        set_kernel_name("maxpool_out_nhwc_bf16x8");
        const long long total = (long long)N * Ho * Wo * (C / 8);
        hipLaunchKernelGGL(maxpool_out_bf16x8_kernel, dim3(pool_grid(total)), dim3(256), 0, st, (const uint4*)x, (uint4*)y, N, H, W, C / 8,
                           Ho, Wo, kh, kw, sh, sw, ph, pw);
    } else {
        set_kernel_name("maxpool_out_nhwc");
        const long long total = (long long)N * Ho * Wo * C;
        if (dtype == MV_BF16)
            hipLaunchKernelGGL(maxpool_out_kernel<bf16_t>, dim3(pool_grid(total)), dim3(256), 0, st, (const bf16_t*)x, (bf16_t*)y, N, H, W,
                               C, Ho, Wo, kh, kw, sh, sw, ph, pw);
        else
            hipLaunchKernelGGL(maxpool_out_kernel<float>, dim3(pool_grid(total)), dim3(256), 0, st, (const float*)x, (float*)y, N, H, W, C,
                               Ho, Wo, kh, kw, sh, sw, ph, pw);
    }
    MV_LAUNCH_CHECK();
    return MV_OK;
}

}  // extern "C"
