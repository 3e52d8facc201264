// The fallback attention kernels (any shape, f32 or bf16; the on-device cross-check of the MFMA kernels under "force_generic") and
// the attention entries that pick between them and the MFMA kernels of attn.hip / swin_attn.hip.  They are NOT the fast path.
#include "mfma_common.h"
#include "swin_geom.h"

namespace mv {

// ------------------------------------------------------------------------------------------
// attention, one wave per (b, h, query): scores and the query in LDS, every K and V row re-read from global memory.
//   ATTN_PLAIN     the N tokens of an image (vit.py:64-73): logits = (q . k) * scale, optional probabilities out
//   ATTN_SWIN      Swin shifted-window attention core (swin.py:123-250): qkv NHWC [B,Hf,Wf,3C] with channel order [q|k|v][head][dh];
//                  roll / partition / reverse / mask are index arithmetic (swin_geom.h); q pre-scaled by dh^-0.5, + bias + mask
//   ATTN_SWIN_COS  Swin V2 (swin.py:159-168): q and k times `rnorm` ([B][2][n][C], swin_qk_rnorm.hip) -- rounded to T like the
//                  operands of the MFMA kernel -- and logit_mul[h] instead of dh^-0.5
// Each mode keeps its own order of floating-point operations.
// ------------------------------------------------------------------------------------------
enum { ATTN_PLAIN = 0, ATTN_SWIN = 1, ATTN_SWIN_COS = 2 };
struct AttnGenericP {
    int n, H, dh;                    // tokens per group (image or window), heads, head width
    float scale;                     // ATTN_PLAIN
    WindowGeom g;                    // ATTN_SWIN*
    const float *bias, *rnorm, *logit_mul;
    float* probs;                    // ATTN_PLAIN, optional
};

template <typename T, int MODE>
__global__ void attn_generic_kernel(const T* __restrict__ qkv, T* __restrict__ out, const AttnGenericP p) {
    extern __shared__ float sm[];  // [n] scores + [dh] q
    constexpr bool SWIN = MODE != ATTN_PLAIN, COS = MODE == ATTN_SWIN_COS;
    const int n = p.n, dh = p.dh, C = p.H * dh;
    float* sc = sm;
    float* qs = sm + n;
    const int h = blockIdx.y, b = blockIdx.z;
    const int lane = threadIdx.x;
    // the query: token blockIdx.x of the image, or of the map in window-major order
    const int nWw = SWIN ? p.g.Wf / p.g.wsw : 1;
    const int win = SWIN ? blockIdx.x / n : 0, ti = SWIN ? blockIdx.x % n : blockIdx.x;
    const int wy = win / nWw, wx = win % nWw;
    auto tok_row = [&](int j) -> long long {           // token j of the group -> its row in qkv / out
        return SWIN ? swin_tok_row(p.g, b, wy, wx, j) : (long long)b * n + j;
    };
    auto region = [&](int j) { return swin_tok_region(p.g, wy, wx, j); };
    const long long rs = 3LL * C;  // row stride of qkv
    const long long orow = tok_row(ti);
    const T* qrow = qkv + orow * rs + h * dh;
    const float qscale = rsqrtf((float)dh);
    auto rnd = [](float v) { return sizeof(T) == 2 ? bf2f(f2bf(v)) : v; };
    const float* rq = COS ? p.rnorm + ((long long)b * 2 * n + ti) * C + h * dh : nullptr;
    for (int d = lane; d < dh; d += 64)
        qs[d] = COS ? rnd(io<T>::ld(qrow + d) * rq[d]) : (SWIN ? io<T>::ld(qrow + d) * qscale : io<T>::ld(qrow + d));
    __syncthreads();
    const bool shifted = SWIN && (p.g.shh + p.g.shw) > 0;
    const int qreg = SWIN ? region(ti) : 0;
    float mx = -INFINITY;
    for (int j = lane; j < n; j += 64) {
        const T* krow = qkv + tok_row(j) * rs + C + h * dh;
        float s = 0.f;
        if (COS) {
            const float* rk = p.rnorm + (((long long)b * 2 + 1) * n + j) * C + h * dh;
            for (int d = 0; d < dh; ++d) s = fmaf(qs[d], rnd(io<T>::ld(krow + d) * rk[d]), s);
            s *= p.logit_mul[h];
        } else {
            for (int d = 0; d < dh; ++d) s = fmaf(qs[d], io<T>::ld(krow + d), s);
            if (!SWIN) s *= p.scale;
        }
        if (SWIN) {
            s += p.bias[((long long)h * n + ti) * n + j];
            if (shifted && region(j) != qreg) s += -100.0f;
        }
        sc[j] = s;
        mx = fmaxf(mx, s);
    }
    mx = wave_max(mx);
    float sum = 0.f;
    for (int j = lane; j < n; j += 64) {
        float e = __expf(sc[j] - mx);
        sc[j] = e;
        sum += e;
    }
    sum = wave_sum(sum);
    __syncthreads();
    const float inv = 1.f / sum;
    if (!SWIN && p.probs) {
        float* pr = p.probs + (((long long)b * p.H + h) * n + ti) * n;
        for (int j = lane; j < n; j += 64) pr[j] = sc[j] * inv;
    }
    for (int d = lane; d < dh; d += 64) {
        float o = 0.f;
        for (int j = 0; j < n; ++j) {
            const T* vrow = qkv + tok_row(j) * rs + 2 * C + h * dh;
            o = fmaf(sc[j], io<T>::ld(vrow + d), o);
        }
        io<T>::st(out + orow * C + h * dh + d, o * inv);
    }
}

// tokens = queries per image; the name reported is the caller's business
template <int MODE>
static int attn_generic_go(const void* qkv, void* out, const AttnGenericP& p, int tokens, int B, int dtype, hipStream_t st) {
    const size_t smem = (size_t)(p.n + p.dh) * sizeof(float);
    const dim3 grid((unsigned)tokens, (unsigned)p.H, (unsigned)B);
    if (dtype == MV_BF16)
        hipLaunchKernelGGL((attn_generic_kernel<bf16_t, MODE>), grid, dim3(64), smem, st, (const bf16_t*)qkv, (bf16_t*)out, p);
    else
        hipLaunchKernelGGL((attn_generic_kernel<float, MODE>), grid, dim3(64), smem, st, (const float*)qkv, (float*)out, p);
    MV_LAUNCH_CHECK();
    return MV_OK;
}

// ------------------------------------------------------------------------------------------
// fp32 attention with the keys and values of one (image, head [, window]) in LDS: the generic kernel above re-reads every K and V row
// from global memory for every query (one wave per query); here a block stages them once (rows padded to dh + 1 floats:
// conflict-free column walks) and its four waves share them.  SWIN: the tokens of a window, gathered through the cyclic shift,
// relative-position bias + region mask (swin.py:90-255); else the N tokens of an image, optional probabilities out (vit.py:64-73).
// The fp32 compute mode and the training step's forward run here.
// ------------------------------------------------------------------------------------------
struct AttnF32P {
    int n, dh, H, C;                 // tokens per group, head width, heads, channels (H * dh)
    WindowGeom g;                    // SWIN only
    float scale;
};
template <bool SWIN>
__global__ __launch_bounds__(SWIN ? 256 : 1024) void attn_f32_lds_kernel(const float* __restrict__ qkv, const float* __restrict__ bias,
                                                           float* __restrict__ out, float* __restrict__ probs, const AttnF32P p) {
    extern __shared__ float sm[];
    const int n = p.n, dh = p.dh, DP = dh + 1, C = p.C;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int NT = SWIN ? 256 : 1024, NW = NT / 64;     // an image's 197 x 64 keys and values fill most of the LDS: one block per CU, so
    float* Ks = sm;                                     // it brings 16 waves; a window's 49 x 32 leave room for several 4-wave blocks
    float* Vs = Ks + n * DP;
    float* sc = Vs + n * DP + wave * (n + dh);          // this wave's scores, then its query
    float* qs = sc + n;
    const int grp = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
    const int nWw = SWIN ? p.g.Wf / p.g.wsw : 1;
    const int wy = SWIN ? grp / nWw : 0, wx = SWIN ? grp - wy * nWw : 0;
    auto tok_row = [&](int j) -> long long {           // token j of the group -> its row in qkv / out
        return SWIN ? swin_tok_row(p.g, b, wy, wx, j) : (long long)b * n + j;
    };
    auto region = [&](int j) { return swin_tok_region(p.g, wy, wx, j); };       // shift-mask region of token j
    const long long rs = 3LL * C;
    for (int idx = tid; idx < n * dh; idx += NT) {
        const int j = idx / dh, d = idx - j * dh;
        const float* r = qkv + tok_row(j) * rs + h * dh + d;
        Ks[j * DP + d] = r[C];
        Vs[j * DP + d] = r[2 * C];
    }
    __syncthreads();
    const bool shifted = SWIN && (p.g.shh + p.g.shw) > 0;
    for (int i = wave; i < n; i += NW) {
        const long long qrow = tok_row(i);
        for (int d = lane; d < dh; d += 64) qs[d] = qkv[qrow * rs + h * dh + d] * p.scale;
        wave_lds_fence();
        const int qreg = shifted ? region(i) : 0;
        float mx = -INFINITY;
        for (int j = lane; j < n; j += 64) {
            float s = 0.f;
            for (int d = 0; d < dh; ++d) s = fmaf(qs[d], Ks[j * DP + d], s);
            if (SWIN) {
                s += bias[((long long)h * n + i) * n + j];
                if (shifted && region(j) != qreg) s += -100.0f;
            }
            sc[j] = s;
            mx = fmaxf(mx, s);
        }
        mx = wave_max(mx);
        float sum = 0.f;
        for (int j = lane; j < n; j += 64) {
            const float e = __expf(sc[j] - mx);
            sc[j] = e;
            sum += e;
        }
        sum = wave_sum(sum);
        const float inv = 1.f / sum;
        wave_lds_fence();
        if (!SWIN && probs)
            for (int j = lane; j < n; j += 64) probs[(((long long)b * p.H + h) * n + i) * n + j] = sc[j] * inv;
        for (int d = lane; d < dh; d += 64) {
            float o = 0.f;
            for (int j = 0; j < n; ++j) o = fmaf(sc[j], Vs[j * DP + d], o);
            out[qrow * C + h * dh + d] = o * inv;
        }
        wave_lds_fence();                               // before the next query overwrites this wave's scores
    }
}
template <bool SWIN>
static int attn_f32_lds_go(const float* qkv, const float* bias, float* out, float* probs, const AttnF32P& p, int groups, int B,
                           hipStream_t st) {
    constexpr int NW = SWIN ? 4 : 16;
    const size_t smem = ((size_t)2 * p.n * (p.dh + 1) + NW * (size_t)(p.n + p.dh)) * sizeof(float);
    auto kern = attn_f32_lds_kernel<SWIN>;
    static LdsAttrSite attr;
    MV_HIP(attr.ensure((const void*)kern, smem));
    hipLaunchKernelGGL(kern, dim3((unsigned)groups, (unsigned)p.H, (unsigned)B), dim3(NW * 64), smem, st, qkv, bias, out, probs, p);
    MV_LAUNCH_CHECK();
    return MV_OK;
}
static bool attn_f32_lds_fits(int n, int dh) {
    return ((size_t)2 * n * (dh + 1) + 16 * (size_t)(n + dh)) * sizeof(float) <= 150 * 1024 && !get_flag("no_attn_f32_lds");
}

}  // namespace mv

using namespace mv;

extern "C" {

int mv_mha_fwd(const void* qkv, void* out, float* probs, int B, int N, int H, int dh, float scale, int dtype,
               mv_stream_t stream) {
    MV_CHECK_ARG(qkv && out && B > 0 && N > 0 && H > 0 && dh > 0, "mha: bad args");
    hipStream_t st = (hipStream_t)stream;
    if (!get_flag("force_generic") && dtype == MV_BF16 && mha_mfma_supported(N, dh, dtype))
        return mha_mfma_launch(qkv, 0, out, probs, B, N, H, dh, scale, nullptr, 1.f, st);
    MV_CHECK_ARG(H <= 65535 && B <= 65535, "mha: H/B too large for the generic kernel");
    if (dtype == MV_F32 && !get_flag("force_generic") && attn_f32_lds_fits(N, dh) && (long long)B * H >= 128) {   // one block per (image, head):
        AttnF32P ap;                                                                                              // fewer do not fill the chip
        memset(&ap, 0, sizeof(ap));
        ap.n = N; ap.dh = dh; ap.H = H; ap.C = H * dh; ap.scale = scale;
        set_kernel_name("mha_f32_lds");
        return attn_f32_lds_go<false>((const float*)qkv, nullptr, (float*)out, probs, ap, 1, B, st);
    }
    MV_CHECK_ARG((size_t)(N + dh) * sizeof(float) <= 64 * 1024, "mha: sequence too long for the generic kernel (N=%d)", N);
    AttnGenericP p;
    memset(&p, 0, sizeof(p));
    p.n = N; p.H = H; p.dh = dh; p.scale = scale; p.probs = probs;
    set_kernel_name("mha_generic");
    return attn_generic_go<ATTN_PLAIN>(qkv, out, p, N, B, dtype, st);
}

int mv_swin_window_attn_fwd(const void* qkv, const float* bias, void* out, int B, int Hf, int Wf, int C, int heads,
                            int ws_h, int ws_w, int shift_h, int shift_w, int dtype, mv_stream_t stream) {
    MV_CHECK_ARG(qkv && bias && out && B > 0 && Hf > 0 && Wf > 0 && C > 0 && heads > 0, "swin_attn: bad args");
    WindowGeom g;
    if (int rc = swin_check_geom("swin_attn", Hf, Wf, C, heads, ws_h, ws_w, shift_h, shift_w, g)) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (!get_flag("force_generic") && swin_mfma_supported(C, heads, ws_h, ws_w, dtype))
        return swin_mfma_launch(qkv, bias, out, B, Hf, Wf, C, heads, ws_h, ws_w, g.shh, g.shw, nullptr, 1.f, st);
    const int n = ws_h * ws_w, dh = C / heads;
    MV_CHECK_ARG(heads <= 65535 && B <= 65535, "swin_attn: grid too large");
    if (dtype == MV_F32 && !get_flag("force_generic") && attn_f32_lds_fits(n, dh)) {
        AttnF32P ap;
        ap.n = n; ap.dh = dh; ap.H = heads; ap.C = C; ap.g = g;
        ap.scale = 1.0f / sqrtf((float)dh);
        set_kernel_name("swin_attn_f32_lds");
        return attn_f32_lds_go<true>((const float*)qkv, bias, (float*)out, nullptr, ap, (Hf / ws_h) * (Wf / ws_w), B, st);
    }
    AttnGenericP p;
    memset(&p, 0, sizeof(p));
    p.n = n; p.H = heads; p.dh = dh; p.g = g; p.bias = bias;
    set_kernel_name("swin_attn_generic");
    return attn_generic_go<ATTN_SWIN>(qkv, out, p, Hf * Wf, B, dtype, st);
}

int mv_swin_window_attn_cos_fwd(const void* qkv, const float* rnorm, const float* logit_mul, const float* bias, void* out,
                                const void* keys, float keep_prob, int B, int Hf, int Wf, int C, int heads, int ws_h, int ws_w,
                                int shift_h, int shift_w, int dtype, mv_stream_t stream) {
    MV_CHECK_ARG(qkv && rnorm && logit_mul && bias && out && B > 0 && Hf > 0 && Wf > 0 && C > 0 && heads > 0, "swin_attn_cos: bad args");
    MV_CHECK_ARG(dtype == MV_BF16 || dtype == MV_F32, "swin_attn_cos: dtype %d", dtype);
    WindowGeom g;
    if (int rc = swin_check_geom("swin_attn_cos", Hf, Wf, C, heads, ws_h, ws_w, shift_h, shift_w, g)) return rc;
    MV_CHECK_ARG(!keys || (keep_prob > 0.f && keep_prob <= 1.f), "swin_attn_cos: keep_prob %g outside (0, 1]", (double)keep_prob);
    hipStream_t st = (hipStream_t)stream;
    const bool mfma = swin_mfma_supported(C, heads, ws_h, ws_w, dtype) != 0;
    if (keys && !mfma) {
        set_error("swin_attn_cos: attention dropout needs bf16, 32 channels per head and <= 64 tokens (C=%d heads=%d window %dx%d dtype=%d)",
                  C, heads, ws_h, ws_w, dtype);
        return MV_E_UNSUPPORTED;
    }
    if (mfma && (keys || !get_flag("force_generic")))
        return swin_mfma_launch(qkv, bias, out, B, Hf, Wf, C, heads, ws_h, ws_w, g.shh, g.shw, (const uint32_t*)keys, keep_prob, st,
                                rnorm, logit_mul);
    const int n = ws_h * ws_w, dh = C / heads;
    MV_CHECK_ARG(heads <= 65535 && B <= 65535, "swin_attn_cos: grid too large");
    MV_CHECK_ARG((size_t)(n + dh) * sizeof(float) <= 64 * 1024, "swin_attn_cos: window too large for the generic kernel (n=%d)", n);
    AttnGenericP p;
    memset(&p, 0, sizeof(p));
    p.n = n; p.H = heads; p.dh = dh; p.g = g; p.bias = bias; p.rnorm = rnorm; p.logit_mul = logit_mul;
    set_kernel_name("swin_attn_generic_cos");
    return attn_generic_go<ATTN_SWIN_COS>(qkv, out, p, Hf * Wf, B, dtype, st);
}

}  // extern "C"
