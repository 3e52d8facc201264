// ShuffleNetV2 unit tail (reference shufflenetv2.py:44-112): depthwise 3x3 + BatchNorm -> 1x1 + BatchNorm + ReLU in ONE launch, and
// the pass-through half of the unit's output in the same launch.  NHWC bf16, gfx950.
//
//   d[m, c] = bf16( dw_scale[c] * sum_{r,s<3} x[b, s*ho + r - 1, s*wo + s' - 1, c] * w_dw[r][s'][c] + dw_shift[c] )      (zero padding)
//   y[m, y_off + n]      = relu( pw_scale[n] * sum_c W[n][c] d[m, c] + pw_shift[n] )   n < N_real;   exact 0 for N_real <= n < N
//   y[m, pass_off + i]   = src[m, phys(i)]   i < n_pass;   exact 0 for n_pass <= i < pass_pad         (bit copy)
//   phys(i) = i / 2 for even i, P_src + i / 2 for odd i   -- the channel shuffle of the previous unit, folded into an index
//
// m is the FLATTENED output pixel index b * Ho * Wo + ho * Wo + wo: a workgroup owns TM = 16 PT consecutive pixels whatever image
// they belong to, so 49-pixel maps fill the machine at batch size.  Three phases, 256 threads:
//   1. the depthwise results of the tile go to LDS as bf16, already in the B-operand fragment order of v_mfma_f32_16x16x32_bf16
//      ([pixel tile][k-step][lane][8]: lane = 16 (c % 32 / 8) + m % 16), so the GEMM's LDS reads are linear 16-byte reads per lane
//      (conflict-free) and the intermediate never reaches HBM.  A thread owns 8 channels of one pixel per item: nine 16-byte loads
//      (neighbouring threads = neighbouring channel chunks; the window is shared through L1 / L2), the nine filter vectors from LDS.
//      Channels Cx .. Kp (Kp = Cx rounded up to the k-step 32) are written as zeros.
//   2. the pass-through copy (two 8-byte loads interleaved into one 16-byte store per 8 channels).
//   3. y^T tile = W . d^T: the weights are the A operand (rows = output channels), streamed from L2 in fragment order (packed once on
//      the host: [N16 tile][k-step][lane][8], lane = 16 (k % 32 / 8) + n % 16, zero rows / columns up to Np x Kp), one 1 KB piece per
//      wave and k-step; a wave owns up to 4 row tiles at a time, so every B fragment read from LDS feeds up to 4 MFMAs.  In the
//      accumulator a lane holds 4 CONSECUTIVE output channels of one pixel: scale, shift, ReLU, one 8-byte store.
// The largest weight matrix (488 x 488: 465 KB) does not fit LDS; it is read once per workgroup from L2.
#include "mfma_common.h"

namespace mv {

namespace {

constexpr int SDP_THREADS = 256;

struct SdpP {
    const bf16_t* x;         // [B][H][W][Cx]
    const bf16_t* w_dw;      // [3][3][Cx]
    const float* dw_scale;   // [Cx] or null
    const float* dw_shift;   // [Cx] or null
    const bf16_t* w_frag;    // [Np / 16][Kp / 32][64][8]
    const float* pw_scale;   // [N] or null
    const float* pw_shift;   // [N] or null
    bf16_t* y;
    const bf16_t* src;       // pass-through source or null
    long long M;             // B * Ho * Wo
    int H, W, Ho, Wo, Cx, Kp, N, N_real, Np, stride;
    int y_pitch, y_off, src_pitch, P_src, n_pass, pass_off, pass_pad;
};

__device__ __forceinline__ void sdp_unpack8(const uint4 u, float* v) {
    v[0] = __uint_as_float(u.x << 16); v[1] = __uint_as_float(u.x & 0xffff0000u);
    v[2] = __uint_as_float(u.y << 16); v[3] = __uint_as_float(u.y & 0xffff0000u);
    v[4] = __uint_as_float(u.z << 16); v[5] = __uint_as_float(u.z & 0xffff0000u);
    v[6] = __uint_as_float(u.w << 16); v[7] = __uint_as_float(u.w & 0xffff0000u);
}

typedef float f32x4 __attribute__((ext_vector_type(4)));

template <int PT>
__global__ __launch_bounds__(SDP_THREADS) void shuffle_dwpw_kernel(const SdpP p) {
    constexpr int TM = 16 * PT;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int KS = p.Kp >> 5, K8 = p.Kp >> 3, C8 = p.Cx >> 3;
    uint4* dl = (uint4*)smem;                                   // [PT][KS][64] fragments of the depthwise tile
    uint4* wl = dl + PT * KS * 64;                              // [9][C8] depthwise filters
    const int tid = threadIdx.x;
    const long long m0 = (long long)blockIdx.x * TM;

    for (int i = tid; i < 9 * C8; i += SDP_THREADS) wl[i] = ((const uint4*)p.w_dw)[i];
    __syncthreads();

    // ---- 1. depthwise 3x3 + folded BatchNorm -> LDS (fragment order)
    for (int i = tid; i < TM * K8; i += SDP_THREADS) {
        const int ml = i / K8, c8 = i - ml * K8;
        const long long m = m0 + ml;
        uint4 out = make_uint4(0, 0, 0, 0);
        if (m < p.M && c8 < C8) {
            const long long bq = m / (p.Ho * p.Wo);
            const int rem = (int)(m - bq * (p.Ho * p.Wo));
            const int ho = rem / p.Wo, wo = rem - ho * p.Wo;
            const int h0 = ho * p.stride - 1, w0 = wo * p.stride - 1;
            const bf16_t* xb = p.x + bq * p.H * p.W * p.Cx + c8 * 8;
            float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const int hi = h0 + r;
                if ((unsigned)hi >= (unsigned)p.H) continue;
#pragma unroll
                for (int s = 0; s < 3; ++s) {
                    const int wi = w0 + s;
                    if ((unsigned)wi >= (unsigned)p.W) continue;
                    float xv[8], wv[8];
                    sdp_unpack8(*(const uint4*)(xb + ((long long)hi * p.W + wi) * p.Cx), xv);
                    sdp_unpack8(wl[(r * 3 + s) * C8 + c8], wv);
#pragma unroll
                    for (int e = 0; e < 8; ++e) acc[e] = fmaf(xv[e], wv[e], acc[e]);
                }
            }
            if (p.dw_scale) {
                const float4 a = *(const float4*)(p.dw_scale + c8 * 8), b2 = *(const float4*)(p.dw_scale + c8 * 8 + 4);
                acc[0] *= a.x; acc[1] *= a.y; acc[2] *= a.z; acc[3] *= a.w; acc[4] *= b2.x; acc[5] *= b2.y; acc[6] *= b2.z; acc[7] *= b2.w;
            }
            if (p.dw_shift) {
                const float4 a = *(const float4*)(p.dw_shift + c8 * 8), b2 = *(const float4*)(p.dw_shift + c8 * 8 + 4);
                acc[0] += a.x; acc[1] += a.y; acc[2] += a.z; acc[3] += a.w; acc[4] += b2.x; acc[5] += b2.y; acc[6] += b2.z; acc[7] += b2.w;
            }
            out.x = pack_bf2(acc[0], acc[1]); out.y = pack_bf2(acc[2], acc[3]);
            out.z = pack_bf2(acc[4], acc[5]); out.w = pack_bf2(acc[6], acc[7]);
        }
        dl[((ml >> 4) * KS + (c8 >> 2)) * 64 + (c8 & 3) * 16 + (ml & 15)] = out;
    }

    // ---- 2. pass-through half: y[m, pass_off + i] = src[m, phys(i)], zeros up to pass_pad
    if (p.src) {
        const int Q8 = p.pass_pad >> 3;
        for (int i = tid; i < TM * Q8; i += SDP_THREADS) {
            const int ml = i / Q8, q = i - ml * Q8;
            const long long m = m0 + ml;
            if (m >= p.M) continue;
            const int i0 = q * 8;
            uint4 out = make_uint4(0, 0, 0, 0);
            if (i0 < p.n_pass) {
                const bf16_t* sp = p.src + m * p.src_pitch + (i0 >> 1);
                const uint2 ev = *(const uint2*)sp, od = *(const uint2*)(sp + p.P_src);       // logical i0, i0+2, .. / i0+1, i0+3, ..
                out.x = (ev.x & 0xffffu) | (od.x << 16);
                out.y = (ev.x >> 16) | (od.x & 0xffff0000u);
                out.z = (ev.y & 0xffffu) | (od.y << 16);
                out.w = (ev.y >> 16) | (od.y & 0xffff0000u);
                const int left = p.n_pass - i0;                   // valid channels of this chunk (>= 1)
                if (left < 8) {
                    unsigned wds[4] = {out.x, out.y, out.z, out.w};
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        if (2 * k >= left) wds[k] = 0;
                        else if (2 * k + 1 >= left) wds[k] &= 0xffffu;
                    }
                    out = make_uint4(wds[0], wds[1], wds[2], wds[3]);
                }
            }
            *(uint4*)(p.y + m * p.y_pitch + p.pass_off + i0) = out;
        }
    }
    __syncthreads();

    // ---- 3. pointwise product on the matrix cores, weights streamed from L2
    const int lane = tid & 63, wave = tid >> 6;
    const int ntiles = p.Np >> 4;
    int G = (ntiles + 3) >> 2;
    G = G > 4 ? 4 : G;
    const int ngroups = (ntiles + G - 1) / G;
    const uint4* wf = (const uint4*)p.w_frag;
    for (int grp = wave; grp < ngroups; grp += SDP_THREADS / 64) {
        const int nt0 = grp * G;
        int cnt = ntiles - nt0;
        cnt = cnt > G ? G : cnt;
        f32x4 acc[4][PT];
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int q = 0; q < PT; ++q) acc[j][q] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
        for (int ks = 0; ks < KS; ++ks) {
            uint4 a[4];
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < cnt) a[j] = wf[((long long)(nt0 + j) * KS + ks) * 64 + lane];
            bf16x8 b[PT];
#pragma unroll
            for (int q = 0; q < PT; ++q) b[q] = __builtin_bit_cast(bf16x8, dl[(q * KS + ks) * 64 + lane]);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (j < cnt) {
                    const bf16x8 av = __builtin_bit_cast(bf16x8, a[j]);
#pragma unroll
                    for (int q = 0; q < PT; ++q) acc[j][q] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av, b[q], acc[j][q], 0, 0, 0);
                }
            }
        }
        // epilogue: lane = (4 consecutive channels n .. n+3, pixel 16 q + lane % 16)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (j >= cnt) continue;
            const int n = (nt0 + j) * 16 + (lane >> 4) * 4;
            if (n >= p.N) continue;
            float4 sc = make_float4(1.f, 1.f, 1.f, 1.f), sf = make_float4(0.f, 0.f, 0.f, 0.f);
            if (p.pw_scale) sc = *(const float4*)(p.pw_scale + n);
            if (p.pw_shift) sf = *(const float4*)(p.pw_shift + n);
#pragma unroll
            for (int q = 0; q < PT; ++q) {
                const long long m = m0 + q * 16 + (lane & 15);
                if (m >= p.M) continue;
                float v0 = fmaxf(fmaf(acc[j][q][0], sc.x, sf.x), 0.f), v1 = fmaxf(fmaf(acc[j][q][1], sc.y, sf.y), 0.f);
                float v2 = fmaxf(fmaf(acc[j][q][2], sc.z, sf.z), 0.f), v3 = fmaxf(fmaf(acc[j][q][3], sc.w, sf.w), 0.f);
                if (n + 0 >= p.N_real) v0 = 0.f;
                if (n + 1 >= p.N_real) v1 = 0.f;
                if (n + 2 >= p.N_real) v2 = 0.f;
                if (n + 3 >= p.N_real) v3 = 0.f;
                uint2 o;
                o.x = pack_bf2(v0, v1);
                o.y = pack_bf2(v2, v3);
                *(uint2*)(p.y + m * p.y_pitch + p.y_off + n) = o;
            }
        }
    }
}

size_t sdp_smem(int PT, int Cx, int Kp) { return (size_t)PT * 16 * Kp * 2 + (size_t)9 * Cx * 2; }

template <int PT>
int sdp_go(const SdpP& p, hipStream_t st) {
    static LdsAttrSite site;
    auto kern = shuffle_dwpw_kernel<PT>;
    const size_t smem = sdp_smem(PT, p.Cx, p.Kp);
    MV_HIP(site.ensure((const void*)kern, smem));
    const long long blocks = (p.M + 16 * PT - 1) / (16 * PT);
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(SDP_THREADS), smem, st, p);
    MV_LAUNCH_CHECK();
    return MV_OK;
}

// y[r, j] = x[r, idx[j]]: one thread per output element (the literal channel shuffle / split of the fallback path)
template <typename T>
__global__ __launch_bounds__(256) void channel_gather_kernel(const T* x, const int* idx, T* y, long long rows, int Cin, int Cout) {
    const long long total = rows * Cout;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long r = i / Cout;
        const int j = (int)(i - r * Cout);
        const int c = idx[j];
        y[i] = (unsigned)c < (unsigned)Cin ? x[r * Cin + c] : (T)0;
    }
}

}  // namespace

}  // namespace mv

extern "C" {

int mv_shuffle_dwpw_supported(int Cx, int N, int stride, int H, int W, int in_dtype, int out_dtype) {
    if (mv::get_flag("no_shuffle_dwpw") || mv::get_flag("force_generic")) return 0;
    if (in_dtype != MV_BF16 || out_dtype != MV_BF16) return 0;
    if (Cx < 8 || Cx > 512 || Cx % 8 || N < 8 || N > 512 || N % 8) return 0;
    if (stride != 1 && stride != 2) return 0;
    return H >= 1 && W >= 1 && H <= 4096 && W <= 4096;
}

int mv_shuffle_dwpw_fwd(const void* x, const void* w_dw, const float* dw_scale, const float* dw_shift, const void* w_frag,
                        const float* pw_scale, const float* pw_shift, void* y, int y_pitch, int y_off, int N, int N_real,
                        const void* src, int src_pitch, int P_src, int n_pass, int pass_off, int pass_pad, int B, int H, int W, int Cx,
                        int stride, int in_dtype, int out_dtype, mv_stream_t stream_) {
    using namespace mv;
    MV_CHECK_ARG(x && w_dw && w_frag && y, "mv_shuffle_dwpw_fwd: NULL argument");
    MV_CHECK_ARG(x != y && src != y, "mv_shuffle_dwpw_fwd: not in place");
    MV_CHECK_ARG(B >= 1, "mv_shuffle_dwpw_fwd: B=%d", B);
    if (!mv_shuffle_dwpw_supported(Cx, N, stride, H, W, in_dtype, out_dtype)) {
        set_error("mv_shuffle_dwpw_fwd: unsupported Cx=%d N=%d stride=%d H=%d W=%d in_dtype=%d out_dtype=%d (ask mv_shuffle_dwpw_supported "
                  "first)", Cx, N, stride, H, W, in_dtype, out_dtype);
        return MV_E_UNSUPPORTED;
    }
    MV_CHECK_ARG(N_real >= 1 && N_real <= N, "mv_shuffle_dwpw_fwd: N_real=%d outside 1 .. N=%d", N_real, N);
    MV_CHECK_ARG(y_pitch % 8 == 0 && y_off % 8 == 0 && y_off >= 0 && y_off + N <= y_pitch,
                 "mv_shuffle_dwpw_fwd: channels y_off=%d .. +N=%d do not fit the pitch %d (multiples of 8)", y_off, N, y_pitch);
    if (src) {
        MV_CHECK_ARG(stride == 1, "mv_shuffle_dwpw_fwd: the pass-through needs stride 1 (one source pixel per output pixel)");
        MV_CHECK_ARG(n_pass >= 1 && pass_pad % 8 == 0 && n_pass <= pass_pad && pass_off % 8 == 0 && pass_off >= 0 &&
                         pass_off + pass_pad <= y_pitch && (pass_off + pass_pad <= y_off || y_off + N <= pass_off),
                     "mv_shuffle_dwpw_fwd: pass-through n_pass=%d pass_off=%d pass_pad=%d does not fit y (pitch %d, product at %d .. +%d)",
                     n_pass, pass_off, pass_pad, y_pitch, y_off, N);
        MV_CHECK_ARG(P_src >= 8 && P_src % 8 == 0 && src_pitch % 8 == 0 && 2 * P_src <= src_pitch && (n_pass + 7) / 8 * 4 <= P_src,
                     "mv_shuffle_dwpw_fwd: pass-through source P_src=%d src_pitch=%d n_pass=%d", P_src, src_pitch, n_pass);
    }
    SdpP p;
    p.x = (const bf16_t*)x; p.w_dw = (const bf16_t*)w_dw; p.dw_scale = dw_scale; p.dw_shift = dw_shift;
    p.w_frag = (const bf16_t*)w_frag; p.pw_scale = pw_scale; p.pw_shift = pw_shift; p.y = (bf16_t*)y; p.src = (const bf16_t*)src;
    p.H = H; p.W = W; p.Ho = (H - 1) / stride + 1; p.Wo = (W - 1) / stride + 1;
    p.M = (long long)B * p.Ho * p.Wo;
    p.Cx = Cx; p.Kp = (Cx + 31) / 32 * 32; p.N = N; p.N_real = N_real; p.Np = (N + 15) / 16 * 16; p.stride = stride;
    p.y_pitch = y_pitch; p.y_off = y_off; p.src_pitch = src_pitch; p.P_src = P_src; p.n_pass = n_pass; p.pass_off = pass_off;
    p.pass_pad = pass_pad;
    MV_CHECK_ARG(p.M <= (1ll << 31), "mv_shuffle_dwpw_fwd: %lld output pixels", p.M);
    hipStream_t st = (hipStream_t)stream_;
    // 64 pixels per workgroup while that leaves two workgroups per CU, else 32, else 16 (49-pixel maps at small batch)
    if (p.M >= 64 * 512) {
        set_kernel_name(stride == 1 ? "shuffle_dwpw_s1_m64" : "shuffle_dwpw_s2_m64");
        return sdp_go<4>(p, st);
    }
    if (p.M >= 32 * 512) {
        set_kernel_name(stride == 1 ? "shuffle_dwpw_s1_m32" : "shuffle_dwpw_s2_m32");
        return sdp_go<2>(p, st);
    }
    set_kernel_name(stride == 1 ? "shuffle_dwpw_s1_m16" : "shuffle_dwpw_s2_m16");
    return sdp_go<1>(p, st);
}

int mv_channel_gather_nhwc_fwd(const void* x, const int* idx, void* y, int64_t rows, int C_in, int C_out, int dtype, mv_stream_t stream_) {
    using namespace mv;
    MV_CHECK_ARG(x && idx && y, "mv_channel_gather_nhwc_fwd: NULL argument");
    MV_CHECK_ARG(x != y, "mv_channel_gather_nhwc_fwd: not in place");
    MV_CHECK_ARG(rows >= 1 && C_in >= 1 && C_out >= 1, "mv_channel_gather_nhwc_fwd: rows=%lld C_in=%d C_out=%d", (long long)rows, C_in, C_out);
    MV_CHECK_ARG(dtype == MV_F32 || dtype == MV_BF16, "mv_channel_gather_nhwc_fwd: dtype %d", dtype);
    hipStream_t st = (hipStream_t)stream_;
    const long long total = (long long)rows * C_out;
    long long g = (total + 255) / 256;
    if (g > 256 * 32) g = 256 * 32;
    set_kernel_name(dtype == MV_F32 ? "channel_gather_f32" : "channel_gather_bf16");
    if (dtype == MV_F32)
        hipLaunchKernelGGL(channel_gather_kernel<float>, dim3((unsigned)g), dim3(256), 0, st, (const float*)x, idx, (float*)y,
                           (long long)rows, C_in, C_out);
    else
        hipLaunchKernelGGL(channel_gather_kernel<bf16_t>, dim3((unsigned)g), dim3(256), 0, st, (const bf16_t*)x, idx, (bf16_t*)y,
                           (long long)rows, C_in, C_out);
    MV_LAUNCH_CHECK();
    return MV_OK;
}

}  // extern "C"
