// eqx.nn.AvgPool2d (reference densenet.py:128: AvgPool2d(kernel_size=2, stride=2) behind a transition's convolution): floor-mode
// output size, no padding, every window full.  NHWC, bf16 or fp32, fp32 sums.  Element-wise and memory-bound: a thread owns 8
// consecutive channels of one output pixel where the channel count allows 16-byte accesses, else one value.
#include "mfma_common.h"

namespace mv {

namespace {

template <typename T, int V>
__global__ __launch_bounds__(256) void avgpool2d_nhwc_kernel(const T* __restrict__ x, T* __restrict__ y, const long long total, const int H,
                                                             const int W, const int CV, const int Ho, const int Wo, const int kh,
                                                             const int kw, const int sh, const int sw) {
    const float inv = 1.0f / (float)(kh * kw);
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int cv = (int)(i % CV);
        long long r = i / CV;
        const int wo = (int)(r % Wo);
        r /= Wo;
        const int ho = (int)(r % Ho);
        const long long b = r / Ho;
        float a[V];
#pragma unroll
        for (int e = 0; e < V; ++e) a[e] = 0.f;
        for (int dy = 0; dy < kh; ++dy)
            for (int dx = 0; dx < kw; ++dx) {
                const T* src = x + (((b * H + ho * sh + dy) * W + wo * sw + dx) * CV + cv) * V;
#pragma unroll
                for (int e = 0; e < V; ++e) a[e] += io<T>::ld(src + e);
            }
#pragma unroll
        for (int e = 0; e < V; ++e) a[e] *= inv;
        if (V == 8) {
            Out8<T>::st(y + i * V, a);
        } else {
            io<T>::st(y + i, a[0]);
        }
    }
}

template <typename T>
void avgpool_go(const void* x, void* y, int N, int H, int W, int C, int Ho, int Wo, int kh, int kw, int sh, int sw, hipStream_t st) {
    const bool vec = C % 8 == 0;
    const int CV = vec ? C / 8 : C;
    const long long total = (long long)N * Ho * Wo * CV;
    const long long blocks = (total + 255) / 256;
    const dim3 grid((unsigned)(blocks < 65536 ? blocks : 65536));
    if (vec)
        hipLaunchKernelGGL((avgpool2d_nhwc_kernel<T, 8>), grid, dim3(256), 0, st, (const T*)x, (T*)y, total, H, W, CV, Ho, Wo, kh, kw, sh,
                           sw);
    else
        hipLaunchKernelGGL((avgpool2d_nhwc_kernel<T, 1>), grid, dim3(256), 0, st, (const T*)x, (T*)y, total, H, W, CV, Ho, Wo, kh, kw, sh,
                           sw);
}

}  // namespace

}  // namespace mv

extern "C" {

int mv_avgpool2d_nhwc_fwd(const void* x, void* y, int N, int H, int W, int C, int kh, int kw, int sh, int sw, int dtype,
                          mv_stream_t stream) {
    using namespace mv;
    MV_CHECK_ARG(x && y && x != y, "mv_avgpool2d_nhwc_fwd: NULL argument or in place");
    MV_CHECK_ARG(N > 0 && C > 0 && kh > 0 && kw > 0 && sh > 0 && sw > 0 && kh * kw <= 4096, "mv_avgpool2d_nhwc_fwd: bad dims");
    MV_CHECK_ARG(H >= kh && W >= kw, "mv_avgpool2d_nhwc_fwd: a %d x %d window on a %d x %d map: empty output", kh, kw, H, W);
    MV_CHECK_ARG(dtype == MV_BF16 || dtype == MV_F32, "mv_avgpool2d_nhwc_fwd: dtype=%d", dtype);
    const int Ho = (H - kh) / sh + 1, Wo = (W - kw) / sw + 1;
    set_kernel_name(C % 8 == 0 ? "avgpool2d_nhwc_x8" : "avgpool2d_nhwc");
    if (dtype == MV_BF16) avgpool_go<bf16_t>(x, y, N, H, W, C, Ho, Wo, kh, kw, sh, sw, (hipStream_t)stream);
    else avgpool_go<float>(x, y, N, H, W, C, Ho, Wo, kh, kw, sh, sw, (hipStream_t)stream);
    MV_LAUNCH_CHECK();
    return MV_OK;
}

}  // extern "C"
