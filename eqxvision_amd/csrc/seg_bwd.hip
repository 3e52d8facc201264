// Backward half of the dense-prediction models (fcn / deeplabv3 / lraspp), gfx950, fp32: the adjoint of the
// bilinear up-sampling of resize.hip and the per-pixel softmax cross entropy over the class axis of NCHW logits.  Both are VALU
// kernels bound by HBM; neither uses an atomic on data, every sum runs in a fixed order (two runs give the same bits).
#include "common.h"

namespace mv {

namespace {

// The two taps of output index o on an axis of `in` source pixels (half-pixel centres, edge clamp; resize.hip: taps_for), as
// weights: w0 on pixel i0, w1 on pixel i1.  On the clamped edges both taps are the edge pixel.  The source coordinate is ONE fused
// multiply-add, written out so that the weights do not depend on the compiler's contraction setting.
struct Tap2 {
    int i0, i1;
    float w0, w1;
};
__device__ __forceinline__ Tap2 tap2(int o, float scale, int in) {
    float src = fmaf((float)o + 0.5f, scale, -0.5f);
    src = src < 0.f ? 0.f : src;                       // first half pixel: all of the weight on pixel 0
    int i0 = (int)src;
    i0 = i0 > in - 1 ? in - 1 : i0;
    const int i1 = i0 + 1 > in - 1 ? in - 1 : i0 + 1;
    const float w1 = src - (float)i0;
    return {i0, i1, 1.0f - w1, w1};
}
// weight of source pixel i in output o: 0 unless one of o's taps is i
__device__ __forceinline__ float weight_on(const Tap2& t, int i) { return (t.i0 == i ? t.w0 : 0.f) + (t.i1 == i ? t.w1 : 0.f); }

// Outputs whose taps can include source pixel i: src(o) in (i - 1, i + 1), i.e. o in ((2i - 1) out / (2 in) - 1/2, (2i + 3) out / (2 in) - 1/2),
// widened by one on both sides (the loop tests every tap, so a range that is too wide costs time, never correctness); the edge pixels
// also collect every clamped output beyond the first / last centre.
__device__ __forceinline__ void footprint(int i, int in, int out, int& lo, int& hi) {
    const long long a = (2LL * i - 1) * out / (2LL * in) - 1, b = (2LL * i + 3) * out / (2LL * in) + 1;
    lo = (i == 0 || a < 0) ? 0 : (int)a;
    hi = (i == in - 1 || b > out - 1) ? out - 1 : (int)b;
}

// Gather form of the adjoint: one thread per dx element sums w_y(oy) w_x(ox) dy[oy, ox] over its footprint, rows outer, columns
// inner, always in that order.  The lanes follow dy's layout, dy being (H W) / (h w) times larger than dx:
//   NCHW dy (what the models return): source column fastest, then source row, channel, image -- at one step of the column loop
//     the lanes of a wave read a run of one dy row W / w elements apart, and over the loop the wave consumes that run whole, so
//     every cache line fetched is used in full; the stores to dx are C elements apart, on the small tensor;
//   NHWC dy: channel fastest -- loads and stores are both contiguous across the wave.
template <bool NCHW>
__global__ __launch_bounds__(256) void resize_bilinear_bwd_kernel(const float* __restrict__ dy, float* __restrict__ dx, int B, int h,
                                                                  int w, int C, int H, int W) {
    const long long total = (long long)B * h * w * C;
    const float sy = (float)h / (float)H, sx = (float)w / (float)W;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        int b, c, iy, ix;
        long long r = idx;
        if (NCHW) {
            ix = (int)(r % w); r /= w;
            iy = (int)(r % h); r /= h;
            c = (int)(r % C); b = (int)(r / C);
        } else {
            c = (int)(r % C); r /= C;
            ix = (int)(r % w); r /= w;
            iy = (int)(r % h); b = (int)(r / h);
        }
        int ylo, yhi, xlo, xhi;
        footprint(iy, h, H, ylo, yhi);
        footprint(ix, w, W, xlo, xhi);
        const float* base = NCHW ? dy + ((long long)b * C + c) * H * W : dy + (long long)b * H * W * C + c;
        const long long ystride = NCHW ? W : (long long)W * C, xstride = NCHW ? 1 : C;
        float acc = 0.f;
        for (int oy = ylo; oy <= yhi; ++oy) {
            const float wy = weight_on(tap2(oy, sy, h), iy);
            if (wy == 0.f) continue;
            const float* row = base + oy * ystride;
            for (int ox = xlo; ox <= xhi; ++ox) {
                const float wx = weight_on(tap2(ox, sx, w), ix);
                if (wx != 0.f) acc = fmaf(wy * wx, row[ox * xstride], acc);
            }
        }
        dx[(((long long)b * h + iy) * w + ix) * C + c] = acc;
    }
}

// Per-pixel cross entropy with integer labels over the class axis of NCHW logits [B, C, HW]: one thread per pixel walks the
// classes (class stride HW), so the lanes of a wave read HW-contiguous logits at every step.  Pass 1 keeps a running maximum and
// the sum of exponentials relative to it (max-subtracted logsumexp in one read), pass 2 writes softmax - onehot.  A pixel that
// `where` masks out gets loss 0 and gradient 0.  A label outside [0, C) on a counted pixel is never used as an index: the pixel is
// treated as masked and bit 1 of the device status word is raised.
__global__ __launch_bounds__(256) void softmax_xent_map_kernel(const float* __restrict__ logits, const int* __restrict__ labels,
                                                               const unsigned char* __restrict__ where, float* __restrict__ loss,
                                                               float* __restrict__ dlogits, unsigned* __restrict__ status, int C,
                                                               long long HW, long long total) {
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        const long long b = idx / HW, p = idx - b * HW;
        const float* l = logits + b * C * HW + p;
        float* d = dlogits + b * C * HW + p;
        const int lab = labels[idx];
        bool counted = where == nullptr || where[idx] != 0;
        if (counted && (unsigned)lab >= (unsigned)C) {
            __hip_atomic_fetch_or(status, 2u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            counted = false;
        }
        if (!counted) {
            loss[idx] = 0.f;
            for (int c = 0; c < C; ++c) d[(long long)c * HW] = 0.f;
            continue;
        }
        float mx = l[0], se = 1.0f, picked = l[0];
        for (int c = 1; c < C; ++c) {
            const float v = l[(long long)c * HW];
            if (c == lab) picked = v;
            if (v > mx) {
                se = se * expf(mx - v) + 1.0f;
                mx = v;
            } else {
                se += expf(v - mx);
            }
        }
        const float lse = mx + logf(se);
        loss[idx] = lse - picked;
        for (int c = 0; c < C; ++c) d[(long long)c * HW] = expf(l[(long long)c * HW] - lse) - (c == lab ? 1.0f : 0.f);
    }
}

// sums[0] = sum of loss, sums[1] = number of counted pixels (counted in integers), in two fixed-order stages inside one block: thread t adds the
// elements t, t + 1024, ... in index order, then the 1024 partial sums are folded pairwise through LDS.
__global__ __launch_bounds__(1024) void xent_map_sums_kernel(const float* __restrict__ loss, const unsigned char* __restrict__ where,
                                                             float* __restrict__ sums, long long total) {
    __shared__ float sl[1024];
    __shared__ unsigned sc[1024];
    float a = 0.f;
    unsigned n = 0;
    for (long long i = threadIdx.x; i < total; i += 1024) {
        a += loss[i];
        n += (where == nullptr || where[i] != 0) ? 1u : 0u;
    }
    sl[threadIdx.x] = a;
    sc[threadIdx.x] = n;
    __syncthreads();
    for (int s = 512; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            sl[threadIdx.x] += sl[threadIdx.x + s];
            sc[threadIdx.x] += sc[threadIdx.x + s];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        sums[0] = sl[0];
        sums[1] = (float)sc[0];
    }
}

inline unsigned grid_of(long long n) {
    const long long g = (n + 255) / 256;
    return (unsigned)(g > 256 * 16 ? 256 * 16 : (g < 1 ? 1 : g));
}

}  // namespace

}  // namespace mv

extern "C" {

using namespace mv;

int mv_resize_bilinear_bwd_nhwc_f32(const float* dy, float* dx, int N, int h, int w, int C, int H, int W, int dy_nchw,
                                    mv_stream_t stream) {
    MV_CHECK_ARG(dy && dx && N > 0 && h > 0 && w > 0 && C > 0 && H > 0 && W > 0, "resize_bilinear_bwd: bad arguments");
    MV_CHECK_ARG(H >= h && W >= w, "resize_bilinear_bwd: %dx%d -> %dx%d is down-sampling; the forward it is the adjoint of only up-samples",
                 h, w, H, W);
    const long long total = (long long)N * h * w * C;
    set_kernel_name(dy_nchw ? "resize_bilinear_bwd_nchw_f32" : "resize_bilinear_bwd_nhwc_f32");
    if (dy_nchw)
        hipLaunchKernelGGL(resize_bilinear_bwd_kernel<true>, dim3(grid_of(total)), dim3(256), 0, (hipStream_t)stream, dy, dx, N, h, w, C,
                           H, W);
    else
        hipLaunchKernelGGL(resize_bilinear_bwd_kernel<false>, dim3(grid_of(total)), dim3(256), 0, (hipStream_t)stream, dy, dx, N, h, w, C,
                           H, W);
    MV_LAUNCH_CHECK();
    return MV_OK;
}

int mv_softmax_xent_map_f32(const float* logits, const int32_t* labels, const uint8_t* where, float* loss, float* dlogits, float* sums,
                            int B, int C, int64_t HW, mv_stream_t stream) {
    MV_CHECK_ARG(logits && labels && loss && dlogits && sums && B > 0 && C > 0 && HW > 0, "softmax_xent_map: bad arguments");
    unsigned* status = device_status_word();
    MV_CHECK_ARG(status != nullptr, "softmax_xent_map: the device status word is not available");
    const long long total = (long long)B * HW;
    MV_CHECK_ARG(total < (1LL << 32), "softmax_xent_map: %lld pixels do not fit the 32-bit pixel count", total);
    set_kernel_name("softmax_xent_map_f32");
    hipLaunchKernelGGL(softmax_xent_map_kernel, dim3(grid_of(total)), dim3(256), 0, (hipStream_t)stream, logits, (const int*)labels, where,
                       loss, dlogits, status, C, (long long)HW, total);
    hipLaunchKernelGGL(xent_map_sums_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, loss, where, sums, total);
    MV_LAUNCH_CHECK();
    return MV_OK;
}

}  // extern "C"
