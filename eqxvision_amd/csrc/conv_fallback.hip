// The any-shape convolution kernels (any size, f32 or bf16) + the convolution / Linear entry points that pick among several
// translation units: they run a route of route.h on the MFMA launchers (conv_launchers.h) or on the kernels below.  An entry that
// wraps ONE translation unit lives in that unit, next to its kernel.
//
// The contraction kernels here are the "any shape" path (odd channel counts such as the
// MlpProjection(20,5,10) of the reference's tests/test_layers.py:25-40) and the on-device
// cross-check for the MFMA kernels (flag "force_generic").  They are NOT the fast path.
#include "conv_launchers.h"
#include "mfma_common.h"

namespace mv {

// ------------------------------------------------------------------------------------------
// direct convolution, one thread per (output row, output channel); x/w addressed by strides so
// the same kernel serves NHWC activations + KRSC weights and NCHW images + OIHW weights.
// ------------------------------------------------------------------------------------------
struct ConvP {
    int N, H, W, C, K, R, S, Ho, Wo, sh, sw, ph, pw, dh, dw, groups;
    long long sxn, sxc, sxh, sxw;  // x strides (elements)
    long long swk, swc, swr, sws;  // w strides (elements)
    int act, tok_stride, tok_offset;
};

template <typename TX, typename TW, typename TY>
__global__ void conv_generic_kernel(const TX* __restrict__ x, const TW* __restrict__ w,
                                    const float* __restrict__ scale, const float* __restrict__ shift,
                                    const TY* __restrict__ residual, TY* __restrict__ y,
                                    const float* __restrict__ pos, ConvP p) {
    const int k = blockIdx.y * blockDim.x + threadIdx.x;
    const long long m = (long long)blockIdx.x * blockDim.y + threadIdx.y;
    const long long M = (long long)p.N * p.Ho * p.Wo;
    if (k >= p.K || m >= M) return;
    const int wo = (int)(m % p.Wo);
    const int ho = (int)((m / p.Wo) % p.Ho);
    const int n = (int)(m / ((long long)p.Wo * p.Ho));
    const int Cg = p.C / p.groups, Kg = p.K / p.groups;
    const int g = k / Kg;
    float acc = 0.f;
    for (int r = 0; r < p.R; ++r) {
        const int hi = ho * p.sh - p.ph + r * p.dh;
        if (hi < 0 || hi >= p.H) continue;
        for (int s = 0; s < p.S; ++s) {
            const int wi = wo * p.sw - p.pw + s * p.dw;
            if (wi < 0 || wi >= p.W) continue;
            const TX* xp = x + n * p.sxn + hi * p.sxh + wi * p.sxw + (long long)(g * Cg) * p.sxc;
            const TW* wp = w + k * p.swk + r * p.swr + s * p.sws;
            for (int c = 0; c < Cg; ++c) acc = fmaf(io<TX>::ld(xp + c * p.sxc), io<TW>::ld(wp + c * p.swc), acc);
        }
    }
    float v = acc;
    if (scale) v *= scale[k];
    if (shift) v += shift[k];
    long long row = m;
    if (p.tok_stride > 0) {
        const int pix = ho * p.Wo + wo;
        row = (long long)n * p.tok_stride + p.tok_offset + pix;
        if (pos) v += pos[(long long)(p.tok_offset + pix) * p.K + k];
    }
    if (residual) v += io<TY>::ld(residual + row * p.K + k);
    v = apply_act_rt(v, p.act);
    io<TY>::st(y + row * p.K + k, v);
}

template <typename TX, typename TW, typename TY>
static int conv_generic_launch(const void* x, const void* w, const float* scale, const float* shift,
                               const void* residual, void* y, const float* pos, const ConvP& p, hipStream_t st) {
    const long long M = (long long)p.N * p.Ho * p.Wo;
    dim3 block(64, 4);
    dim3 grid((unsigned)((M + 3) / 4), (p.K + 63) / 64);
    hipLaunchKernelGGL((conv_generic_kernel<TX, TW, TY>), grid, block, 0, st, (const TX*)x, (const TW*)w, scale, shift,
                       (const TY*)residual, (TY*)y, pos, p);
    MV_LAUNCH_CHECK();
    return MV_OK;
}

// ------------------------------------------------------------------------------------------
// the same contraction in fp32 on the matrix cores (v_mfma_f32_32x32x2_f32): the fp32 compute mode and the training step (both
// passes run in fp32) spend their time here.  One wave = 32 output channels x 32 output positions; A = weights (lane: channel fr,
// reduction element fh), B = the positions' input rows; a lane loads FOUR consecutive reduction channels at once (its half of a group
// of eight), which feeds four MFMA steps when the reduction index is contiguous in both operands (channels-last); any other layout
// (the NCHW image + OIHW filter of the entry convolutions) takes two strided scalars per step.  groups = 1.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void conv_f32_mfma_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                            const float* __restrict__ scale, const float* __restrict__ shift,
                                                            const float* __restrict__ residual, float* __restrict__ y,
                                                            const float* __restrict__ pos, ConvP p) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, fr = lane & 31, fh = lane >> 5;
    const long long M = (long long)p.N * p.Ho * p.Wo;
    const long long m = ((long long)blockIdx.x * 4 + wave) * 32 + fr;
    const int k0 = blockIdx.y * 32;
    const bool mok = m < M;
    const long long mm = mok ? m : 0;
    const int wo = (int)(mm % p.Wo), ho = (int)((mm / p.Wo) % p.Ho), n = (int)(mm / ((long long)p.Wo * p.Ho));
    const bool kok = k0 + fr < p.K;
    const float* wk = w + (long long)(kok ? k0 + fr : 0) * p.swk;
    const bool vec = p.sxc == 1 && p.swc == 1 && (p.C & 3) == 0 && (p.sxn & 3) == 0 && (p.sxh & 3) == 0 && (p.sxw & 3) == 0 &&
                     (p.swk & 3) == 0 && (p.swr & 3) == 0 && (p.sws & 3) == 0;
    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
    for (int r = 0; r < p.R; ++r) {
        const int hi = ho * p.sh - p.ph + r * p.dh;
        for (int s_ = 0; s_ < p.S; ++s_) {
            const int wi = wo * p.sw - p.pw + s_ * p.dw;
            const bool inside = mok && (unsigned)hi < (unsigned)p.H && (unsigned)wi < (unsigned)p.W;
            const float* xp = x + (inside ? n * p.sxn + hi * p.sxh + wi * p.sxw : 0);
            const float* wp = wk + r * p.swr + s_ * p.sws;
            if (vec) {
                for (int c0 = 0; c0 < p.C; c0 += 8) {
                    const int c = c0 + 4 * fh;
                    const bool cin = c < p.C;                                    // C % 8 == 4: the upper half of the last group is empty
                    const float4 a = (kok && cin) ? *(const float4*)(wp + c) : make_float4(0.f, 0.f, 0.f, 0.f);
                    const float4 b = (inside && cin) ? *(const float4*)(xp + c) : make_float4(0.f, 0.f, 0.f, 0.f);
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, acc, 0, 0, 0);
                }
            } else {
                for (int c0 = 0; c0 < p.C; c0 += 2) {
                    const int c = c0 + fh;
                    const bool cin = c < p.C;
                    const float a = (kok && cin) ? wp[c * p.swc] : 0.f;       // any layout: NCHW images + OIHW filters (the entry convolutions)
                    const float b = (inside && cin) ? xp[c * p.sxc] : 0.f;
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
                }
            }
        }
    }
    if (!mok) return;
    long long row = m;
    int pix = 0;
    if (p.tok_stride > 0) {
        pix = ho * p.Wo + wo;
        row = (long long)n * p.tok_stride + p.tok_offset + pix;
    }
    // acc[4 q + i]: channel k0 + 8 q + 4 fh + i of position fr
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int k = k0 + 8 * q + 4 * fh + i;
            if (k >= p.K) continue;
            float v = acc[4 * q + i];
            if (scale) v *= scale[k];
            if (shift) v += shift[k];
            if (p.tok_stride > 0 && pos) v += pos[(long long)(p.tok_offset + pix) * p.K + k];
            if (residual) v += residual[row * p.K + k];
            v = apply_act_rt(v, p.act);
            y[row * p.K + k] = v;
        }
}

// The same contraction with both operands staged through LDS: a block = 64 channels x 256 positions, eight waves of 64 x 32 (two MFMA
// tiles each); the reduction runs in chunks of 32 channels of one filter tap: 8 KB of weights + 32 KB of input rows per chunk, fetched
// as whole 128-byte rows (eight lanes per row), double-buffered (the next chunk travels global -> registers while this one
// multiplies, then registers -> LDS behind one barrier).  Rows are padded to 36 floats: conflict-free ds_read_b128 fragments.
// Needs 16-byte-aligned rows (C and all strides multiples of 4); dispatched from 64 reduction channels per tap up (with four waves per
// block it only paid from 128; eight waves: resnet50 fp32 4291 -> 5097 img/s, vit_base 1414 -> 1585, swin_t 3214 -> 3697).
__global__ __launch_bounds__(512) void conv_f32_lds_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                           const float* __restrict__ scale, const float* __restrict__ shift,
                                                           const float* __restrict__ residual, float* __restrict__ y,
                                                           const float* __restrict__ pos, ConvP p) {
    constexpr int RP = 36, WROWS = 64, XROWS = 256, STAGE = (WROWS + XROWS) * RP;       // floats per stage
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 31, fh = lane >> 5;
    const long long M = (long long)p.N * p.Ho * p.Wo;
    const long long m0 = (long long)blockIdx.x * XROWS;
    const int k0 = blockIdx.y * WROWS;
    // loader role: thread t fetches float4 number (t & 7) of rows (t >> 3) + 64 i (eight waves: two per SIMD)
    const int lrow = tid >> 3, lq = tid & 7;
    int xn[4], xho[4], xwo[4];
    bool xok[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const long long m = m0 + lrow + 64 * i;
        xok[i] = m < M;
        const long long mm = xok[i] ? m : 0;
        xwo[i] = (int)(mm % p.Wo); xho[i] = (int)((mm / p.Wo) % p.Ho); xn[i] = (int)(mm / ((long long)p.Wo * p.Ho));
    }
    const int cpt = (p.C + 31) / 32;                                   // chunks per filter tap
    const int nchunk = p.R * p.S * cpt;
    float4 gx[4], gw;
    auto fetch = [&](int ch) {
        const int tap = ch / cpt, c0 = (ch - tap * cpt) * 32 + 4 * lq;
        const int r = tap / p.S, s_ = tap - r * p.S;
        const bool cin = c0 < p.C;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int hi = xho[i] * p.sh - p.ph + r * p.dh, wi = xwo[i] * p.sw - p.pw + s_ * p.dw;
            const bool in = xok[i] && cin && (unsigned)hi < (unsigned)p.H && (unsigned)wi < (unsigned)p.W;
            gx[i] = in ? *(const float4*)(x + xn[i] * p.sxn + hi * p.sxh + wi * p.sxw + c0) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        {
            const int k = k0 + lrow;
            gw = (k < p.K && cin) ? *(const float4*)(w + (long long)k * p.swk + r * p.swr + s_ * p.sws + c0) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    auto stash = [&](int buf) {
        float* base = lds + buf * STAGE;
        *(float4*)(base + lrow * RP + 4 * lq) = gw;
#pragma unroll
        for (int i = 0; i < 4; ++i) *(float4*)(base + (WROWS + lrow + 64 * i) * RP + 4 * lq) = gx[i];
    };
    f32x16 acc[2];                                                     // a wave: 64 channels x 32 positions
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[a][e] = 0.f;
    fetch(0);
    stash(0);
    __syncthreads();
    for (int ch = 0; ch < nchunk; ++ch) {
        const int buf = ch & 1;
        if (ch + 1 < nchunk) fetch(ch + 1);
        const float* wl = lds + buf * STAGE + fr * RP + 4 * fh;
        const float* xl = lds + buf * STAGE + (WROWS + 32 * wave + fr) * RP + 4 * fh;
#pragma unroll
        for (int j = 0; j < 4; ++j) {                                   // 8 reduction channels per step: a lane holds its half of 4
            float4 a[2];
            const float4 b = *(const float4*)(xl + 8 * j);
#pragma unroll
            for (int t = 0; t < 2; ++t) a[t] = *(const float4*)(wl + 32 * t * RP + 8 * j);
#pragma unroll
            for (int kt = 0; kt < 2; ++kt) {
                acc[kt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[kt].x, b.x, acc[kt], 0, 0, 0);
                acc[kt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[kt].y, b.y, acc[kt], 0, 0, 0);
                acc[kt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[kt].z, b.z, acc[kt], 0, 0, 0);
                acc[kt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[kt].w, b.w, acc[kt], 0, 0, 0);
            }
        }
        if (ch + 1 < nchunk) {
            stash(buf ^ 1);                                             // its last reader finished before the previous barrier
            __syncthreads();
        }
    }
    // epilogue: acc[kt][4 q + i] = channel k0 + 32 kt + 8 q + 4 fh + i of position m0 + 32 wave + fr
    {
        const long long m = m0 + 32 * wave + fr;
        if (m >= M) return;
        long long row = m;
        int pix = 0;
        if (p.tok_stride > 0) {
            const int wo = (int)(m % p.Wo), ho = (int)((m / p.Wo) % p.Ho), n = (int)(m / ((long long)p.Wo * p.Ho));
            pix = ho * p.Wo + wo;
            row = (long long)n * p.tok_stride + p.tok_offset + pix;
        }
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int k = k0 + 32 * kt + 8 * q + 4 * fh + i;
                    if (k >= p.K) continue;
                    float v = acc[kt][4 * q + i];
                    if (scale) v *= scale[k];
                    if (shift) v += shift[k];
                    if (p.tok_stride > 0 && pos) v += pos[(long long)(p.tok_offset + pix) * p.K + k];
                    if (residual) v += residual[row * p.K + k];
                    v = apply_act_rt(v, p.act);
                    y[row * p.K + k] = v;
                }
    }
}

static int conv_generic_dispatch(const void* x, const void* w, const float* scale, const float* shift,
                                 const void* residual, void* y, const float* pos, const ConvP& p, int x_dtype,
                                 int w_dtype, int y_dtype, hipStream_t st) {
    const long long M = (long long)p.N * p.Ho * p.Wo;
    const bool aligned4 = p.sxc == 1 && p.swc == 1 && (p.C & 3) == 0 && (p.sxn & 3) == 0 && (p.sxh & 3) == 0 && (p.sxw & 3) == 0 &&
                          (p.swk & 3) == 0 && (p.swr & 3) == 0 && (p.sws & 3) == 0;
    const int variant = generic_variant(x_dtype == MV_F32 && w_dtype == MV_F32 && y_dtype == MV_F32, p.groups, p.C, p.K, aligned4, M, get_flag);
    set_kernel_name(generic_kernel_name(variant));
    if (variant == 2) {
        constexpr int SMEM = 2 * (64 + 256) * 36 * 4;
        static LdsAttrSite attr;
        MV_HIP(attr.ensure((const void*)conv_f32_lds_kernel, SMEM));
        hipLaunchKernelGGL(conv_f32_lds_kernel, dim3((unsigned)((M + 255) / 256), (unsigned)((p.K + 63) / 64)), dim3(512), SMEM, st,
                           (const float*)x, (const float*)w, scale, shift, (const float*)residual, (float*)y, pos, p);
        MV_LAUNCH_CHECK();
        return MV_OK;
    }
    if (variant == 1) {
        hipLaunchKernelGGL(conv_f32_mfma_kernel, dim3((unsigned)((M + 127) / 128), (unsigned)((p.K + 31) / 32)), dim3(256), 0, st,
                           (const float*)x, (const float*)w, scale, shift, (const float*)residual, (float*)y, pos, p);
        MV_LAUNCH_CHECK();
        return MV_OK;
    }
#define GO(TX, TW, TY) return conv_generic_launch<TX, TW, TY>(x, w, scale, shift, residual, y, pos, p, st)
    if (x_dtype == MV_F32 && w_dtype == MV_F32 && y_dtype == MV_F32) GO(float, float, float);
    if (x_dtype == MV_BF16 && w_dtype == MV_BF16 && y_dtype == MV_BF16) GO(bf16_t, bf16_t, bf16_t);
    if (x_dtype == MV_BF16 && w_dtype == MV_BF16 && y_dtype == MV_F32) GO(bf16_t, bf16_t, float);
    if (x_dtype == MV_F32 && w_dtype == MV_BF16 && y_dtype == MV_BF16) GO(float, bf16_t, bf16_t);
    if (x_dtype == MV_F32 && w_dtype == MV_F32 && y_dtype == MV_BF16) GO(float, float, bf16_t);
#undef GO
    set_error("conv: unsupported dtype combination x=%d w=%d y=%d", x_dtype, w_dtype, y_dtype);
    return MV_E_UNSUPPORTED;
}

// Executes a route of route_conv / route_linear (route.h): the matrix-core launchers, or this file's generic kernels.
static int conv_route_launch(const void* x, const void* w, const float* scale, const float* shift, const void* residual, void* y,
                             const ConvShape& s, Route r, hipStream_t st) {
    if (r.kern == Kern::skinny && r.tile == 1) {              // fp32 classifier heads (exact-fp32 MFMA)
        set_kernel_name(kernel_name(r, true, s, false, false, get_flag));
        return skinny_f32_launch(x, w, scale, shift, y, s.M(), s.C, s.K, s.act, st);
    }
    if (r.kern != Kern::generic) return igemm_launch(x, w, scale, shift, residual, y, s, r, st);
    ConvP p;
    p.N = s.N; p.H = s.H; p.W = s.W; p.C = s.C; p.K = s.K; p.R = s.R; p.S = s.S; p.Ho = s.Ho(); p.Wo = s.Wo();
    p.sh = s.sh; p.sw = s.sw; p.ph = s.ph; p.pw = s.pw; p.dh = s.dh; p.dw = s.dw; p.groups = s.groups;
    p.sxn = (long long)s.H * s.W * s.C; p.sxh = (long long)s.W * s.C; p.sxw = s.C; p.sxc = 1;
    const int Cg = s.C / s.groups;
    p.swk = (long long)s.R * s.S * Cg; p.swr = (long long)s.S * Cg; p.sws = Cg; p.swc = 1;
    p.act = s.act; p.tok_stride = 0; p.tok_offset = 0;
    return conv_generic_dispatch(x, w, scale, shift, residual, y, nullptr, p, s.in_dtype, s.in_dtype, s.out_dtype, st);
}

}  // namespace mv

using namespace mv;

extern "C" {

int mv_conv2d_nhwc_fwd(const void* x, const void* w, const float* scale, const float* shift, const void* residual,
                       void* y, int N, int H, int W, int C, int K, int R, int S, int sh, int sw, int ph, int pw,
                       int dh, int dw, int groups, int act, int in_dtype, int out_dtype, mv_stream_t stream) {
    MV_CHECK_ARG(act >= MV_ACT_NONE && act <= MV_ACT_SILU, "conv2d_nhwc: unknown activation %d", act);
    MV_CHECK_ARG(x && w && y, "conv2d_nhwc: NULL pointer");
    MV_CHECK_ARG(N > 0 && H > 0 && W > 0 && C > 0 && K > 0 && R > 0 && S > 0, "conv2d_nhwc: non-positive dims");
    MV_CHECK_ARG(sh > 0 && sw > 0 && dh > 0 && dw > 0 && ph >= 0 && pw >= 0, "conv2d_nhwc: bad stride/dilation/pad");
    MV_CHECK_ARG(groups > 0 && C % groups == 0 && K % groups == 0, "conv2d_nhwc: C=%d K=%d not divisible by groups=%d",
                 C, K, groups);
    const ConvShape s = {N, H, W, C, K, R, S, sh, sw, ph, pw, dh, dw, groups, act, in_dtype, out_dtype, residual != nullptr, scale != nullptr};
    MV_CHECK_ARG(s.Ho() > 0 && s.Wo() > 0, "conv2d_nhwc: empty output (%d x %d)", s.Ho(), s.Wo());
    return conv_route_launch(x, w, scale, shift, residual, y, s, route_conv(s, get_flag), (hipStream_t)stream);
}

int mv_conv2d_nchw_fwd(const void* x, const void* w, const float* scale, const float* shift, void* y, int N, int C,
                       int H, int W, int K, int R, int S, int sh, int sw, int ph, int pw, int act, int x_dtype,
                       int out_dtype, int tok_stride, int tok_offset, const float* pos, mv_stream_t stream) {
    MV_CHECK_ARG(act >= MV_ACT_NONE && act <= MV_ACT_SILU, "conv2d_nchw: unknown activation %d", act);   // every epilogue of this entry has them all
    MV_CHECK_ARG(x && w && y, "conv2d_nchw: NULL pointer");
    MV_CHECK_ARG(N > 0 && H > 0 && W > 0 && C > 0 && K > 0 && R > 0 && S > 0, "conv2d_nchw: non-positive dims");
    MV_CHECK_ARG(sh > 0 && sw > 0 && ph >= 0 && pw >= 0, "conv2d_nchw: bad stride/pad");
    const int Ho = (H + 2 * ph - (R - 1) - 1) / sh + 1;
    const int Wo = (W + 2 * pw - (S - 1) - 1) / sw + 1;
    MV_CHECK_ARG(Ho > 0 && Wo > 0, "conv2d_nchw: empty output");
    MV_CHECK_ARG(tok_stride == 0 || tok_stride >= tok_offset + Ho * Wo, "conv2d_nchw: tok_stride too small");
    hipStream_t st = (hipStream_t)stream;
    if (!get_flag("force_generic") && stem_supported(C, K, R, S, x_dtype, out_dtype))
        return stem_launch(x, w, scale, shift, y, N, C, H, W, K, R, S, sh, sw, ph, pw, act, x_dtype, out_dtype,
                           tok_stride, tok_offset, pos, st);
    ConvP p;
    p.N = N; p.H = H; p.W = W; p.C = C; p.K = K; p.R = R; p.S = S; p.Ho = Ho; p.Wo = Wo;
    p.sh = sh; p.sw = sw; p.ph = ph; p.pw = pw; p.dh = 1; p.dw = 1; p.groups = 1;
    p.sxn = (long long)C * H * W; p.sxc = (long long)H * W; p.sxh = W; p.sxw = 1;
    p.swk = (long long)C * R * S; p.swc = (long long)R * S; p.swr = S; p.sws = 1;
    p.act = act; p.tok_stride = tok_stride; p.tok_offset = tok_offset;
    return conv_generic_dispatch(x, w, scale, shift, nullptr, y, pos, p, x_dtype, out_dtype, out_dtype, st);
}

int mv_conv1x1_chain_supported(int64_t M, int C, int K, int N2, int dtype) {
    return !get_flag("force_generic") && !get_flag("no_stream") &&
           (chain1x1_supported(M, C, K, N2, dtype) || chain_stream_supported(M, C, K, N2, dtype));
}

int mv_conv1x1_chain_fwd(const void* x, const void* w3, const float* scale3, const float* shift3, const void* residual,
                         void* y, const void* w1, const float* scale1, const float* shift1, void* t1, int64_t M, int C,
                         int K, int N2, int dtype, mv_stream_t stream) {
    MV_CHECK_ARG(x && w3 && residual && y && w1 && t1, "conv1x1_chain: NULL pointer");
    if (!mv_conv1x1_chain_supported(M, C, K, N2, dtype)) {
        set_error("conv1x1_chain: unsupported shape M=%lld C=%d K=%d N2=%d (ask mv_conv1x1_chain_supported first)",
                  (long long)M, C, K, N2);
        return MV_E_UNSUPPORTED;
    }
    MV_CHECK_ARG(y != residual && y != x && t1 != y, "conv1x1_chain: y must not alias x / residual / t1");
    if (chain_stream_supported(M, C, K, N2, dtype))        // weights streamed through LDS (layer2's 128 -> 512 -> 128)
        return chain_stream_launch(x, w3, scale3, shift3, residual, y, w1, scale1, shift1, t1, M, (hipStream_t)stream);
    return chain1x1_launch(x, w3, scale3, shift3, residual, y, w1, scale1, shift1, t1, M, N2, (hipStream_t)stream);
}

int mv_conv1x1_chain_res_supported(int N, int H, int W, int C, int K, int N2, int sub, int dtype) {
    return !get_flag("force_generic") && !get_flag("no_stream") && N > 0 && H > 0 && W > 0 &&
           (chain_res_supported(N, H, W, C, K, N2, sub, dtype) || chain_l2_res_supported(N, H, W, C, K, N2, sub, dtype));
}

int mv_conv1x1_chain_res_fwd(const void* t2, const void* residual, const void* wfrag, const void* shifts, void* y, void* t1, int N, int H,
                             int W, int C, int K, int N2, int sub, int dtype, mv_stream_t stream) {
    MV_CHECK_ARG(t2 && residual && wfrag && shifts && y && t1, "conv1x1_chain_res: NULL pointer");
    if (!mv_conv1x1_chain_res_supported(N, H, W, C, K, N2, sub, dtype)) {
        set_error("conv1x1_chain_res: unsupported shape N=%d H=%d W=%d C=%d K=%d N2=%d sub=%d (ask mv_conv1x1_chain_res_supported first)", N,
                  H, W, C, K, N2, sub);
        return MV_E_UNSUPPORTED;
    }
    MV_CHECK_ARG(y != residual && y != t2 && t1 != y && t1 != residual && t1 != t2, "conv1x1_chain_res: outputs must not alias inputs");
    if (C == 128)                                          // C = 128 / K = 512 (layer 2): weights streamed through LDS (chain_l2.hip)
        return chain_l2_res_launch(t2, residual, wfrag, shifts, y, t1, N, H, W, N2, sub, (hipStream_t)stream);
    return chain_res_launch(t2, residual, wfrag, shifts, y, t1, N, H, W, sub, (hipStream_t)stream);
}

int mv_conv1x1_dual_chain_res_supported(int64_t M, int C1, int C2, int K, int N2, int dtype) {
    return !get_flag("force_generic") && !get_flag("no_stream") && chain_l2_dual_supported(M, C1, C2, K, N2, dtype);
}

int mv_conv1x1_dual_chain_res_fwd(const void* t2, const void* x, const void* wfrag, const void* shifts, void* y, void* t1, int64_t M,
                                  int C1, int C2, int K, int N2, int dtype, mv_stream_t stream) {
    MV_CHECK_ARG(t2 && x && wfrag && shifts && y && t1, "conv1x1_dual_chain_res: NULL pointer");
    if (!mv_conv1x1_dual_chain_res_supported(M, C1, C2, K, N2, dtype)) {
        set_error("conv1x1_dual_chain_res: unsupported shape M=%lld C1=%d C2=%d K=%d N2=%d (ask mv_conv1x1_dual_chain_res_supported first)",
                  (long long)M, C1, C2, K, N2);
        return MV_E_UNSUPPORTED;
    }
    MV_CHECK_ARG(y != t2 && y != x && t1 != y && t1 != t2 && t1 != x, "conv1x1_dual_chain_res: outputs must not alias inputs");
    return chain_l2_dual_launch(t2, x, wfrag, shifts, y, t1, M, (hipStream_t)stream);
}

int mv_conv1x1_dual_supported(int64_t M, int C1, int C2, int K, int dtype) {
    return conv1x1_dual_supported(M, C1, C2, K, dtype, get_flag);
}

int mv_conv1x1_dual_fwd(const void* x, const void* x2, const void* wcat, const float* scale, const float* shift, void* y,
                        int N, int Ho, int Wo, int C1, int H2, int W2, int C2, int stride2, int K, int act, int dtype,
                        mv_stream_t stream) {
    MV_CHECK_FUSED_ACT(act, "conv1x1_dual");
    MV_CHECK_ARG(x && x2 && wcat && y, "conv1x1_dual: NULL pointer");
    MV_CHECK_ARG(N > 0 && Ho > 0 && Wo > 0 && stride2 >= 1 && (Ho - 1) * stride2 < H2 && (Wo - 1) * stride2 < W2,
                 "conv1x1_dual: the strided source does not cover the output map");
    const int64_t M = (int64_t)N * Ho * Wo;
    const Route r = route_conv1x1_dual(M, C1, C2, K, stride2, dtype, get_flag);
    if (r.tile == 0) {
        set_error("conv1x1_dual: unsupported shape M=%lld C1=%d C2=%d K=%d (ask mv_conv1x1_dual_supported first)", (long long)M,
                  C1, C2, K);
        return MV_E_UNSUPPORTED;
    }
    ConvShape s = linear_shape(M, K, C1, act, MV_BF16, MV_BF16, false, scale != nullptr);
    set_kernel_name(kernel_name(r, true, s, true, false, get_flag));
    if (r.kern == Kern::igemm8)
        return igemm8_dual_launch(x, x2, wcat, scale, shift, nullptr, y, N, Ho, Wo, C1, H2, W2, C2, stride2, K, act, MV_BF16, r.tile,
                                  (hipStream_t)stream);
    return igemm2_dual_launch(x, x2, wcat, scale, shift, y, N, Ho, Wo, C1, H2, W2, C2, stride2, K, act, r.tile, (hipStream_t)stream);
}

int mv_conv1x1_dual_chain_supported(int64_t M, int C1, int C2, int K, int N2, int dtype) {
    return !get_flag("force_generic") && !get_flag("no_stream") && chain1x1_dual_supported(M, C1, C2, K, N2, dtype);
}

int mv_conv1x1_dual_chain_fwd(const void* x, const void* x2, const void* wcat, const float* scale, const float* shift, void* y,
                              const void* w1, const float* scale1, const float* shift1, void* t1, int64_t M, int C1, int C2,
                              int K, int N2, int dtype, mv_stream_t stream) {
    MV_CHECK_ARG(x && x2 && wcat && w1 && t1, "conv1x1_dual_chain: NULL pointer");       // y may be NULL: the block output is not stored
    if (!mv_conv1x1_dual_chain_supported(M, C1, C2, K, N2, dtype)) {
        set_error("conv1x1_dual_chain: unsupported shape M=%lld C1=%d C2=%d K=%d N2=%d (ask mv_conv1x1_dual_chain_supported)",
                  (long long)M, C1, C2, K, N2);
        return MV_E_UNSUPPORTED;
    }
    return chain1x1_dual_launch(x, x2, wcat, scale, shift, y, w1, scale1, shift1, t1, M, (hipStream_t)stream);
}

int mv_linear_fwd(const void* x, const void* w, const float* scale, const float* shift, const void* residual,
                  void* y, int64_t M, int N, int K, int act, int in_dtype, int out_dtype, mv_stream_t stream) {
    MV_CHECK_FUSED_ACT(act, "linear");
    MV_CHECK_ARG(x && w && y, "linear: NULL pointer");
    MV_CHECK_ARG(M > 0 && N > 0 && K > 0 && M < (1LL << 31), "linear: bad dims M=%lld N=%d K=%d", (long long)M, N, K);
    const ConvShape s = linear_shape(M, N, K, act, in_dtype, out_dtype, residual != nullptr, scale != nullptr);
    return conv_route_launch(x, w, scale, shift, residual, y, s, route_linear(s, get_flag), (hipStream_t)stream);
}

int mv_linear_split_supported(int64_t M, int N, int K, int dtype) {
    return dtype == MV_BF16 && !get_flag("force_generic") && M < (1LL << 31) - 256 &&
           igemm8_supported(M, K, N, 1, 1, 2LL * M * K, 4LL * N * K) && K % 64 == 0;
}

int mv_linear_split_fwd(const void* x, const void* w_hi_lo, const float* scale, const float* shift, const void* residual,
                        void* y, int64_t M, int N, int K, int act, int in_dtype, int out_dtype, mv_stream_t stream) {
    MV_CHECK_FUSED_ACT(act, "linear_split");
    MV_CHECK_ARG(x && w_hi_lo && y, "linear_split: NULL pointer");
    if (!mv_linear_split_supported(M, N, K, in_dtype)) {
        set_error("linear_split: unsupported shape M=%lld N=%d K=%d (ask mv_linear_split_supported first)", (long long)M, N, K);
        return MV_E_UNSUPPORTED;
    }
    const Route r = route_linear_split(M, N, K, get_flag);
    set_kernel_name(kernel_name(r, true, linear_shape(M, N, K, act, in_dtype, out_dtype, residual != nullptr, scale != nullptr), true, false, get_flag));
    // the second reduction source IS x: [x | x] . [w_hi | w_lo]^T = x . (w_hi + w_lo)^T, accumulated in fp32
    return igemm8_dual_launch(x, x, w_hi_lo, scale, shift, residual, y, 1, (int)M, 1, K, (int)M, 1, K, 1, N, act, out_dtype, r.tile,
                              (hipStream_t)stream);
}

int mv_linear_heads_supported(int64_t M, int N, int K, int tokens, int dh, int dtype) {
    return dtype == MV_BF16 && dh == 64 && N % 64 == 0 && K % 64 == 0 && tokens > 0 && M > 0 && M % tokens == 0 &&
           M < (1LL << 31) - 256 && igemm2_wanted(M, K, N, 1, 1) && !get_flag("force_generic") && !get_flag("no_igemm2") &&
           mha_mfma_supported(tokens, dh, dtype);
}

int mv_linear_heads_fwd(const void* x, const void* w, const float* scale, const float* shift, void* y, int64_t M, int N,
                        int K, int tokens, int dh, int dtype, mv_stream_t stream) {
    MV_CHECK_ARG(x && w && y, "linear_heads: NULL pointer");
    if (!mv_linear_heads_supported(M, N, K, tokens, dh, dtype)) {
        set_error("linear_heads: unsupported shape M=%lld N=%d K=%d tokens=%d dh=%d (ask mv_linear_heads_supported first)",
                  (long long)M, N, K, tokens, dh);
        return MV_E_UNSUPPORTED;
    }
    const Route r = route_linear_heads(M, N, K, get_flag);
    const ConvShape s = linear_shape(M, N, K, MV_ACT_NONE, MV_BF16, MV_BF16, false, scale != nullptr);
    set_kernel_name(kernel_name(r, true, s, false, false, get_flag));
    if (r.kern == Kern::igemm8) return igemm8_launch(x, w, scale, shift, nullptr, y, s, tokens, r.tile, (hipStream_t)stream);
    return igemm2_launch(x, w, scale, shift, nullptr, y, s, r.tile, tokens, (hipStream_t)stream);
}

}  // extern "C"
