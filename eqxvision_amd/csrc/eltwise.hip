// Element-wise, per-channel, cast, layout and gather kernels (HBM-bound VALU passes) and their entries.
#include "mfma_common.h"

namespace mv {

template <typename T>
__global__ void eltwise_kernel(const T* __restrict__ x, T* __restrict__ y, long long n, int act) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        io<T>::st(y + i, apply_act_rt(io<T>::ld(x + i), act));
}
template <typename T>
__global__ void add_kernel(const T* __restrict__ a, const T* __restrict__ b, T* __restrict__ y, long long n,
                           int act) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        io<T>::st(y + i, apply_act_rt(io<T>::ld(a + i) + io<T>::ld(b + i), act));
}
template <typename T>
__global__ void channel_scale_kernel(const T* __restrict__ x, const T* __restrict__ sc, T* __restrict__ y, long long HW, int C,
                                     long long n) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        const long long b = i / ((long long)C * HW);
        io<T>::st(y + i, io<T>::ld(x + i) * io<T>::ld(sc + b * C + c));
    }
}
// The element-wise passes with 8 values (16 bytes in bf16) per thread: what the SqueezeExcitation multiply, the un-fused activations
// (hard_swish after a kernel that does not fuse it) and the un-fused residual adds of the section-8 f1 families run on.  HBM-bound;
// the one-value-per-thread kernels above reach 1.9 TB/s, these > 5.
template <typename T> __device__ __forceinline__ void ld8(const T* p, float* v) {
    const float4 a = Out4<T>::ld(p), b = Out4<T>::ld(p + 4);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}
template <typename T>
__global__ void eltwise_vec8_kernel(const T* __restrict__ x, T* __restrict__ y, long long n8, int act) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (long long)gridDim.x * blockDim.x) {
        float v[8];
        ld8(x + i * 8, v);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = apply_act_rt(v[e], act);
        Out8<T>::st(y + i * 8, v);
    }
}
template <typename T>
__global__ void add_vec8_kernel(const T* __restrict__ a, const T* __restrict__ b, T* __restrict__ y, long long n8, int act) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (long long)gridDim.x * blockDim.x) {
        float v[8], w[8];
        ld8(a + i * 8, v);
        ld8(b + i * 8, w);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = apply_act_rt(v[e] + w[e], act);
        Out8<T>::st(y + i * 8, v);
    }
}
template <typename T>
__global__ void channel_scale_vec8_kernel(const T* __restrict__ x, const T* __restrict__ sc, T* __restrict__ y, long long HW, int C,
                                          long long n8) {
    const long long V = C >> 3;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (long long)gridDim.x * blockDim.x) {
        const long long pix = i / V;
        const int c = (int)(i - pix * V) * 8;
        const long long b = pix / HW;
        float v[8], w[8];
        ld8(x + i * 8, v);
        ld8(sc + b * C + c, w);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] *= w[e];
        Out8<T>::st(y + i * 8, v);
    }
}
static inline int grid_vec8(long long n8) {
    const long long g = (n8 + 255) / 256;
    return (int)(g > 256 * 32 ? 256 * 32 : (g < 1 ? 1 : g));
}

template <typename T>
__global__ void channel_affine_kernel(const T* __restrict__ x, const float* __restrict__ scale,
                                      const float* __restrict__ shift, T* __restrict__ y, long long rows, int C,
                                      int act) {
    const long long n = rows * C;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        float v = io<T>::ld(x + i);
        if (scale) v *= scale[c];
        if (shift) v += shift[c];
        io<T>::st(y + i, apply_act_rt(v, act));
    }
}
// 8 consecutive channels per thread (16-byte accesses in bf16), optional residual: y = act(x * scale[c] + shift[c] + residual) --
// the normalisation pass of a training-mode BatchNorm (every convolution output goes through it once: HBM-bound)
template <typename T>
__global__ void channel_affine_vec8_kernel(const T* __restrict__ x, const float* __restrict__ scale, const float* __restrict__ shift,
                                           const T* __restrict__ residual, T* __restrict__ y, long long n8, int C, int act) {
    const int V = C >> 3;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (long long)gridDim.x * blockDim.x) {
        const int c = (int)((unsigned long long)i % (unsigned)V) * 8;
        const T* p = x + i * 8;
        const float4 a = Out4<T>::ld(p), b = Out4<T>::ld(p + 4);
        float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
        float4 s0 = make_float4(1.f, 1.f, 1.f, 1.f), s1 = s0, h0 = make_float4(0.f, 0.f, 0.f, 0.f), h1 = h0;
        if (scale) { s0 = *(const float4*)(scale + c); s1 = *(const float4*)(scale + c + 4); }      // c % 8 == 0: 32-byte aligned
        if (shift) { h0 = *(const float4*)(shift + c); h1 = *(const float4*)(shift + c + 4); }
        const float sc[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
        const float sh[8] = {h0.x, h0.y, h0.z, h0.w, h1.x, h1.y, h1.z, h1.w};
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = fmaf(v[e], sc[e], sh[e]);
        if (residual) {
            const float4 ra = Out4<T>::ld(residual + i * 8), rb = Out4<T>::ld(residual + i * 8 + 4);
            const float r[8] = {ra.x, ra.y, ra.z, ra.w, rb.x, rb.y, rb.z, rb.w};
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] += r[e];
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = apply_act_rt(v[e], act);
        Out8<T>::st(y + i * 8, v);
    }
}

template <typename TI, typename TO>
__global__ void cast_kernel(const TI* __restrict__ x, TO* __restrict__ y, long long n) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        io<TO>::st(y + i, io<TI>::ld(x + i));
}

// NCHW <-> NHWC through a 32x33 LDS tile over (C, HW) so both sides stay coalesced.
template <typename TI, typename TO, bool TO_NHWC>
__global__ void layout_kernel(const TI* __restrict__ x, TO* __restrict__ y, int C, int HW) {
    __shared__ float tile[32][33];
    const int n = blockIdx.z;
    const int c0 = blockIdx.y * 32, p0 = blockIdx.x * 32;
    const int tx = threadIdx.x, ty = threadIdx.y;  // 32 x 8
    const TI* xs = x + (long long)n * C * HW;
    TO* ys = y + (long long)n * C * HW;
    if (TO_NHWC) {  // read [c][p] rows (p contiguous), write [p][c] rows (c contiguous)
        for (int j = ty; j < 32; j += 8) {
            const int c = c0 + j, p = p0 + tx;
            if (c < C && p < HW) tile[j][tx] = io<TI>::ld(xs + (long long)c * HW + p);
        }
        __syncthreads();
        for (int j = ty; j < 32; j += 8) {
            const int p = p0 + j, c = c0 + tx;
            if (c < C && p < HW) io<TO>::st(ys + (long long)p * C + c, tile[tx][j]);
        }
    } else {
        for (int j = ty; j < 32; j += 8) {
            const int p = p0 + j, c = c0 + tx;
            if (c < C && p < HW) tile[j][tx] = io<TI>::ld(xs + (long long)p * C + c);
        }
        __syncthreads();
        for (int j = ty; j < 32; j += 8) {
            const int c = c0 + j, p = p0 + tx;
            if (c < C && p < HW) io<TO>::st(ys + (long long)c * HW + p, tile[tx][j]);
        }
    }
}

template <typename T>
__global__ void cls_pos_kernel(const float* __restrict__ cls, const float* __restrict__ pos, T* __restrict__ tok,
                               int B, int tok_stride, int D) {
    const long long n = (long long)B * D;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += (long long)gridDim.x * blockDim.x) {
        const int d = (int)(i % D);
        const int b = (int)(i / D);
        io<T>::st(tok + (long long)b * tok_stride * D + d, cls[d] + pos[d]);
    }
}

template <typename T>
__global__ void patch_merge_kernel(const T* __restrict__ x, T* __restrict__ y, int B, int H, int W, int C) {
    const int Ho = (H + 1) / 2, Wo = (W + 1) / 2;
    const long long n = (long long)B * Ho * Wo * 4 * C;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += (long long)gridDim.x * blockDim.x) {
        const int c4 = (int)(i % (4 * C));
        long long m = i / (4 * C);
        const int wo = (int)(m % Wo);
        m /= Wo;
        const int ho = (int)(m % Ho);
        const int b = (int)(m / Ho);
        const int q = c4 / C, c = c4 % C;
        // block order [ (0::2,0::2) | (1::2,0::2) | (0::2,1::2) | (1::2,1::2) ]  (swin.py:26-30)
        const int hi = 2 * ho + (q & 1), wi = 2 * wo + (q >> 1);
        float v = 0.f;
        if (hi < H && wi < W) v = io<T>::ld(x + (((long long)b * H + hi) * W + wi) * C + c);
        io<T>::st(y + i, v);
    }
}

// 16-byte chunks: c16 = chunks per source pixel (C * sizeof(T) / 16); y rows are [4 * c16] chunks
__global__ void patch_merge_vec_kernel(const uint4* __restrict__ x, uint4* __restrict__ y, int B, int H, int W, int c16) {
    const int Ho = (H + 1) / 2, Wo = (W + 1) / 2;
    const long long n = (long long)B * Ho * Wo * 4 * c16;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += (long long)gridDim.x * blockDim.x) {
        const int c4 = (int)(i % (4 * c16));
        long long m = i / (4 * c16);
        const int wo = (int)(m % Wo);
        m /= Wo;
        const int ho = (int)(m % Ho);
        const int b = (int)(m / Ho);
        const int q = c4 / c16, c = c4 - q * c16;
        const int hi = 2 * ho + (q & 1), wi = 2 * wo + (q >> 1);
        uint4 v = make_uint4(0, 0, 0, 0);
        if (hi < H && wi < W) v = x[(((long long)b * H + hi) * W + wi) * c16 + c];
        y[i] = v;
    }
}

}  // namespace mv

using namespace mv;

extern "C" {

int mv_patch_merge_gather_nhwc(const void* x, void* y, int B, int H, int W, int C, int dtype, mv_stream_t stream) {
    MV_CHECK_ARG(x && y && B > 0 && H > 0 && W > 0 && C > 0, "patch_merge: bad args");
    hipStream_t st = (hipStream_t)stream;
    const long long n = (long long)B * ((H + 1) / 2) * ((W + 1) / 2) * 4 * C;
    return dispatch_dtype("patch_merge", dtype, [&](auto t) -> int {
        using T = decltype(t);
        const int esz = (int)sizeof(T);
        if ((C * esz) % 16 == 0 && !get_flag("force_generic")) {
            set_kernel_name("patch_merge_gather_vec");
            const int c16 = C * esz / 16;
            const long long nv = (long long)B * ((H + 1) / 2) * ((W + 1) / 2) * 4 * c16;
            hipLaunchKernelGGL(patch_merge_vec_kernel, dim3(grid_for(nv)), dim3(256), 0, st, (const uint4*)x, (uint4*)y, B, H, W,
                               c16);
        } else {
            set_kernel_name("patch_merge_gather");
            hipLaunchKernelGGL(patch_merge_kernel<T>, dim3(grid_for(n)), dim3(256), 0, st, (const T*)x, (T*)y, B, H, W, C);
        }
        MV_LAUNCH_CHECK();
        return MV_OK;
    });
}

int mv_vit_cls_pos_fwd(const float* cls, const float* pos, void* tokens, int B, int tok_stride, int D, int dtype,
                       mv_stream_t stream) {
    MV_CHECK_ARG(cls && pos && tokens && B > 0 && tok_stride > 0 && D > 0, "cls_pos: bad args");
    hipStream_t st = (hipStream_t)stream;
    const long long n = (long long)B * D;
    set_kernel_name("vit_cls_pos");
    return dispatch_dtype("cls_pos", dtype, [&](auto t) -> int {
        using T = decltype(t);
        hipLaunchKernelGGL(cls_pos_kernel<T>, dim3(grid_for(n)), dim3(256), 0, st, cls, pos, (T*)tokens, B, tok_stride, D);
        MV_LAUNCH_CHECK();
        return MV_OK;
    });
}

int mv_eltwise_fwd(const void* x, void* y, int64_t n, int act, int dtype, mv_stream_t stream) {
    MV_CHECK_ARG(x && y && n > 0, "eltwise: bad args");
    hipStream_t st = (hipStream_t)stream;
    return dispatch_dtype("eltwise", dtype, [&](auto t) -> int {
        using T = decltype(t);
        if (n % 8 == 0 && !get_flag("eltwise_scalar")) {
            set_kernel_name("eltwise_x8");
            hipLaunchKernelGGL(eltwise_vec8_kernel<T>, dim3(grid_vec8(n / 8)), dim3(256), 0, st, (const T*)x, (T*)y, (long long)(n / 8),
                               act);
        } else {
            set_kernel_name("eltwise");
            hipLaunchKernelGGL(eltwise_kernel<T>, dim3(grid_for(n)), dim3(256), 0, st, (const T*)x, (T*)y, (long long)n, act);
        }
        MV_LAUNCH_CHECK();
        return MV_OK;
    });
}

int mv_channel_scale_nhwc_fwd(const void* x, const void* sc, void* y, int N, int64_t HW, int C, int dtype, mv_stream_t stream) {
    MV_CHECK_ARG(x && sc && y && N > 0 && HW > 0 && C > 0, "channel_scale: bad args");
    hipStream_t st = (hipStream_t)stream;
    const long long n = (long long)N * HW * C;
    return dispatch_dtype("channel_scale", dtype, [&](auto t) -> int {
        using T = decltype(t);
        if (C % 8 == 0 && !get_flag("eltwise_scalar")) {
            set_kernel_name("channel_scale_x8");
            hipLaunchKernelGGL(channel_scale_vec8_kernel<T>, dim3(grid_vec8(n / 8)), dim3(256), 0, st, (const T*)x, (const T*)sc, (T*)y,
                               (long long)HW, C, n / 8);
        } else {
            set_kernel_name("channel_scale");
            hipLaunchKernelGGL(channel_scale_kernel<T>, dim3(grid_for(n)), dim3(256), 0, st, (const T*)x, (const T*)sc, (T*)y,
                               (long long)HW, C, n);
        }
        MV_LAUNCH_CHECK();
        return MV_OK;
    });
}

int mv_add_fwd(const void* a, const void* b, void* y, int64_t n, int act, int dtype, mv_stream_t stream) {
    MV_CHECK_ARG(a && b && y && n > 0, "add: bad args");
    hipStream_t st = (hipStream_t)stream;
    return dispatch_dtype("add", dtype, [&](auto t) -> int {
        using T = decltype(t);
        if (n % 8 == 0 && !get_flag("eltwise_scalar")) {
            set_kernel_name("add_x8");
            hipLaunchKernelGGL(add_vec8_kernel<T>, dim3(grid_vec8(n / 8)), dim3(256), 0, st, (const T*)a, (const T*)b, (T*)y,
                               (long long)(n / 8), act);
        } else {
            set_kernel_name("add");
            hipLaunchKernelGGL(add_kernel<T>, dim3(grid_for(n)), dim3(256), 0, st, (const T*)a, (const T*)b, (T*)y, (long long)n, act);
        }
        MV_LAUNCH_CHECK();
        return MV_OK;
    });
}

static int channel_affine_go(const char* who, const void* x, const float* scale, const float* shift, const void* residual, void* y,
                             int64_t rows, int C, int act, int dtype, hipStream_t st) {
    const long long n = (long long)rows * C;
    return dispatch_dtype(who, dtype, [&](auto t) -> int {
        using T = decltype(t);
        if (C % 8 == 0 && !get_flag("affine_scalar")) {      // 16-byte accesses; the scalar kernel serves odd widths (and residual-free calls only)
            const long long n8 = n / 8;
            long long g = (n8 + 255) / 256;
            const int grid = (int)(g > 256 * 32 ? 256 * 32 : g);
            set_kernel_name(residual ? "channel_affine_res_x8" : "channel_affine_x8");
            hipLaunchKernelGGL(channel_affine_vec8_kernel<T>, dim3(grid), dim3(256), 0, st, (const T*)x, scale, shift, (const T*)residual,
                               (T*)y, n8, C, act);
            MV_LAUNCH_CHECK();
            return MV_OK;
        }
        if (residual) {
            set_error("channel_affine_res: C=%d is not a multiple of 8", C);
            return MV_E_UNSUPPORTED;
        }
        set_kernel_name("channel_affine");
        hipLaunchKernelGGL(channel_affine_kernel<T>, dim3(grid_for(n)), dim3(256), 0, st, (const T*)x, scale, shift, (T*)y,
                           (long long)rows, C, act);
        MV_LAUNCH_CHECK();
        return MV_OK;
    });
}

int mv_channel_affine_fwd(const void* x, const float* scale, const float* shift, void* y, int64_t rows, int C,
                          int act, int dtype, mv_stream_t stream) {
    MV_CHECK_ARG(x && y && rows > 0 && C > 0, "channel_affine: bad args");
    return channel_affine_go("channel_affine", x, scale, shift, nullptr, y, rows, C, act, dtype, (hipStream_t)stream);
}

// y = act(x * scale[c] + shift[c] + residual): BatchNorm's normalisation + the block's identity + ReLU in one pass (the tail of a
// residual block whose BatchNorm is in training mode and therefore not in the convolution's epilogue; resnet.py:155-160)
int mv_channel_affine_res_fwd(const void* x, const float* scale, const float* shift, const void* residual, void* y, int64_t rows, int C,
                              int act, int dtype, mv_stream_t stream) {
    MV_CHECK_ARG(x && y && residual && rows > 0 && C > 0, "channel_affine_res: bad args");
    return channel_affine_go("channel_affine_res", x, scale, shift, residual, y, rows, C, act, dtype, (hipStream_t)stream);
}

static int layout_launch(const char* who, const void* x, void* y, int N, int C, int H, int W, int in_dtype, int out_dtype, bool to_nhwc,
                         hipStream_t st) {
    const int HW = H * W;
    dim3 block(32, 8), grid((HW + 31) / 32, (C + 31) / 32, N);
    return dispatch_io(who, in_dtype, out_dtype, [&](auto ti, auto to) -> int {
        using TI = decltype(ti); using TO = decltype(to);
        if (to_nhwc)
            hipLaunchKernelGGL((layout_kernel<TI, TO, true>), grid, block, 0, st, (const TI*)x, (TO*)y, C, HW);
        else
            hipLaunchKernelGGL((layout_kernel<TI, TO, false>), grid, block, 0, st, (const TI*)x, (TO*)y, C, HW);
        MV_LAUNCH_CHECK();
        return MV_OK;
    });
}

int mv_nchw_to_nhwc(const void* x, void* y, int N, int C, int H, int W, int in_dtype, int out_dtype,
                    mv_stream_t stream) {
    MV_CHECK_ARG(x && y && N > 0 && C > 0 && H > 0 && W > 0 && N <= 65535, "nchw_to_nhwc: bad args");
    set_kernel_name("nchw_to_nhwc");
    return layout_launch("nchw_to_nhwc", x, y, N, C, H, W, in_dtype, out_dtype, true, (hipStream_t)stream);
}
int mv_nhwc_to_nchw(const void* x, void* y, int N, int C, int H, int W, int in_dtype, int out_dtype,
                    mv_stream_t stream) {
    MV_CHECK_ARG(x && y && N > 0 && C > 0 && H > 0 && W > 0 && N <= 65535, "nhwc_to_nchw: bad args");
    set_kernel_name("nhwc_to_nchw");
    return layout_launch("nhwc_to_nchw", x, y, N, C, H, W, in_dtype, out_dtype, false, (hipStream_t)stream);
}

int mv_cast(const void* x, void* y, int64_t n, int in_dtype, int out_dtype, mv_stream_t stream) {
    MV_CHECK_ARG(x && y && n > 0, "cast: bad args");
    hipStream_t st = (hipStream_t)stream;
    set_kernel_name("cast");
    return dispatch_io("cast", in_dtype, out_dtype, [&](auto ti, auto to) -> int {
        using TI = decltype(ti); using TO = decltype(to);
        hipLaunchKernelGGL((cast_kernel<TI, TO>), dim3(grid_for(n)), dim3(256), 0, st, (const TI*)x, (TO*)y, (long long)n);
        MV_LAUNCH_CHECK();
        return MV_OK;
    });
}

}  // extern "C"
