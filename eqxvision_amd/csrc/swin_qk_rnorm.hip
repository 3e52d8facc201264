// Swin V2 cosine attention, the normalisation (reference `_shifted_window_attention` with logit_scale, swin.py:159-163):
//     q / jnp.linalg.norm(q, ord=2, axis=0),  q of shape (nW, heads, n, dh)
// Axis 0 is the WINDOWS of one image, not the feature axis; the quirk is kept.  So there is one norm per
// (q or k, token-in-window t, channel c):   rnorm[b][s][t][c] = 1 / sqrt(sum over the nW windows w of x_s[w][t][c]^2)
// with the windows taken from the rolled, partitioned map -- the same token walk as swin_attn.hip's tok_row, shift included.
//
// Memory-bound: one thread per (image, q / k, token, 16-byte channel chunk) walks the windows in increasing order with one 16-byte
// load each and accumulates in fp32; neighbouring threads read neighbouring chunks of one qkv row.  Two thirds of qkv are read once,
// the value third never.  No atomics: the order of the sum is fixed.  A zero norm gives inf (and NaN logits), as in the reference.
#include "common.h"

namespace mv {

template <typename T> struct Chunk16;
template <> struct Chunk16<bf16_t> {
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
template <> struct Chunk16<float> {
    static constexpr int N = 4;
    __device__ static __forceinline__ void ld(const float* p, float* v) {
        const float4 u = *(const float4*)p;
        v[0] = u.x; v[1] = u.y; v[2] = u.z; v[3] = u.w;
    }
};

struct RnormP {
    int B, Hf, Wf, C, wsh, wsw, shh, shw, n, nWw, nW, nch;
    long long total;            // B * 2 * n * nch threads
};

template <typename T>
__global__ __launch_bounds__(256) void swin_qk_rnorm_kernel(const T* __restrict__ qkv, float* __restrict__ rnorm, const RnormP p) {
    constexpr int N = Chunk16<T>::N;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= p.total) return;
    const int ch = (int)(i % p.nch);
    long long r = i / p.nch;
    const int t = (int)(r % p.n);
    r /= p.n;
    const int s = (int)(r & 1), b = (int)(r >> 1);
    const int ty = t / p.wsw, tx = t - ty * p.wsw;
    const long long rs = 3LL * p.C;
    const T* base = qkv + (long long)s * p.C + ch * N;
    float acc[N];
#pragma unroll
    for (int e = 0; e < N; ++e) acc[e] = 0.f;
    for (int wy = 0; wy < p.Hf / p.wsh; ++wy) {
        int oy = wy * p.wsh + ty + p.shh;
        if (oy >= p.Hf) oy -= p.Hf;
        for (int wx = 0; wx < p.nWw; ++wx) {          // window index wy * nWw + wx: increasing order
            int ox = wx * p.wsw + tx + p.shw;
            if (ox >= p.Wf) ox -= p.Wf;
            float v[N];
            Chunk16<T>::ld(base + (((long long)b * p.Hf + oy) * p.Wf + ox) * rs, v);
#pragma unroll
            for (int e = 0; e < N; ++e) acc[e] = fmaf(v[e], v[e], acc[e]);
        }
    }
    float* dst = rnorm + (((long long)b * 2 + s) * p.n + t) * p.C + ch * N;
#pragma unroll
    for (int e = 0; e < N; e += 4)
        *(float4*)(dst + e) = make_float4(1.0f / sqrtf(acc[e]), 1.0f / sqrtf(acc[e + 1]), 1.0f / sqrtf(acc[e + 2]), 1.0f / sqrtf(acc[e + 3]));
}

static int swin_qk_rnorm_launch(const void* qkv, float* rnorm, int B, int Hf, int Wf, int C, int ws_h, int ws_w, int shift_h,
                                int shift_w, int dtype, hipStream_t st) {
    RnormP p;
    p.B = B; p.Hf = Hf; p.Wf = Wf; p.C = C; p.wsh = ws_h; p.wsw = ws_w; p.shh = shift_h; p.shw = shift_w;
    p.n = ws_h * ws_w;
    p.nWw = Wf / ws_w;
    p.nW = (Hf / ws_h) * p.nWw;
    p.nch = C / (dtype == MV_BF16 ? 8 : 4);
    p.total = (long long)B * 2 * p.n * p.nch;
    const long long blocks = (p.total + 255) / 256;
    if (blocks >= (1LL << 31)) {
        set_error("swin_qk_rnorm: grid too large");
        return MV_E_UNSUPPORTED;
    }
    set_kernel_name("swin_qk_rnorm");
    if (dtype == MV_BF16)
        hipLaunchKernelGGL(swin_qk_rnorm_kernel<bf16_t>, dim3((unsigned)blocks), dim3(256), 0, st, (const bf16_t*)qkv, rnorm, p);
    else
        hipLaunchKernelGGL(swin_qk_rnorm_kernel<float>, dim3((unsigned)blocks), dim3(256), 0, st, (const float*)qkv, rnorm, p);
    MV_LAUNCH_CHECK();
    return MV_OK;
}

}  // namespace mv

using namespace mv;

extern "C" int mv_swin_qk_rnorm_fwd(const void* qkv, float* rnorm, int B, int Hf, int Wf, int C, int ws_h, int ws_w, int shift_h,
                                    int shift_w, int dtype, mv_stream_t stream) {
    MV_CHECK_ARG(qkv && rnorm && B > 0 && Hf > 0 && Wf > 0 && C > 0, "swin_qk_rnorm: bad args");
    MV_CHECK_ARG(dtype == MV_BF16 || dtype == MV_F32, "swin_qk_rnorm: dtype %d", dtype);
    MV_CHECK_ARG(ws_h > 0 && ws_w > 0 && shift_h >= 0 && shift_w >= 0 && shift_h < ws_h && shift_w < ws_w, "swin_qk_rnorm: bad window / shift");
    if (Hf % ws_h || Wf % ws_w) {
        set_error("swin_qk_rnorm: feature map %dx%d is not a multiple of the window %dx%d (reference swin.py:782-790)", Hf, Wf, ws_h, ws_w);
        return MV_E_UNSUPPORTED;
    }
    if (C % (dtype == MV_BF16 ? 8 : 4)) {
        set_error("swin_qk_rnorm: C=%d is not a whole number of 16-byte chunks", C);
        return MV_E_UNSUPPORTED;
    }
    if (ws_h >= Hf) shift_h = 0;  // swin.py:116-120
    if (ws_w >= Wf) shift_w = 0;
    return swin_qk_rnorm_launch(qkv, rnorm, B, Hf, Wf, C, ws_h, ws_w, shift_h, shift_w, dtype, (hipStream_t)stream);
}
