// DenseNet's pre-activated pointwise convolution (reference densenet.py:63-64, 116-130): BatchNorm + ReLU in FRONT of a 1x1 convolution,
// with an optional 2 x 2 average in front of the product and a strided source and destination.  NHWC bf16, fp32 accumulation on the
// matrix cores, gfx950.
//
//   a[mo, c] = bf16( mean over the p x p window of  relu(s1[c] * x[pix * ldx + c] + h1[c]) )     c < C,  p in {1, 2}
//   v[mo, n] = sum_c w[n][c] * a[mo, c]
//   y[mo * ldy + cy + n] = relu(s2[n] * v + h2[n]),  or v itself when s2 == h2 == NULL
//
// The pre-activation cannot be folded into whatever produced x: every consumer of a DenseNet feature has its own statistics.  It is
// applied to the B operand on its way into LDS instead.  With p = 2 the output map is floor(H / 2) x floor(W / 2) (AvgPool2d(2, 2): an
// odd last row or column is dropped).  The reference pools AFTER the convolution; both are linear, so the average in front is exact
// algebra -- sum_c w[n][c] mean_window(r) == mean_window(sum_c w[n][c] r) -- and the transition's product runs over a quarter of the
// pixels.  The mean is taken in fp32 after affine + ReLU and before the one rounding to bf16.
//
// Rows of x are ldx >= C elements apart and only channels [0, C) of a row are ever read: the rest of a dense block's buffer is memory
// that a later layer has not written yet.  The tile, the chunk loop and the epilogue walk are pw128.h's; a B-operand row is made of
// P x P source pixels held in registers while the matrix cores work, and the affine step, the ReLU, the mean and the rounding happen
// when those registers are written to LDS, behind the chunk's MFMAs.  Reduction channels past C and rows past M must be ZERO AFTER
// the pre-activation, and relu(0 * s + h) is not zero: they are masked behind the affine step (zeros are written to LDS) and are
// never loaded.
#include "pw128.h"

namespace mv {

namespace {

struct PreactP {
    const bf16_t* x;       // [B][H][W] rows of ldx
    const bf16_t* w;       // [N][C]
    const float* s1;       // [C]
    const float* h1;       // [C]
    const float* s2;       // [N] or null (identity)
    const float* h2;
    bf16_t* y;
    long long M, ldx, ldy; // M = B * Ho * Wo output pixels
    int C, N, cy, H, W, Ho, Wo;
};

__device__ __forceinline__ void preact_acc8(float (&a)[8], const uint4 v, const float (&s)[8], const float (&h)[8]) {
    const uint32_t u[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        a[2 * i] += fmaxf(fmaf(__uint_as_float(u[i] << 16), s[2 * i], h[2 * i]), 0.f);
        a[2 * i + 1] += fmaxf(fmaf(__uint_as_float(u[i] & 0xffff0000u), s[2 * i + 1], h[2 * i + 1]), 0.f);
    }
}

// the B operand: a pixel row is made of the P x P source pixels src[j] + {0, 1} + {0, W}, pre-activated on their way into LDS
template <int P>
struct PreactRows {
    const PreactP& p;
    const PwStageMap map;
    long long src[4];
    bool row_ok[4];
    uint4 xr[4][P * P];
    float sv[8], hv[8];
    bool kok;
    __device__ __forceinline__ void init() {
        kok = false;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long long m = pw128_m0() + map.sr + 32 * j;
            row_ok[j] = m < p.M;
            if (P == 1) {
                src[j] = m;
            } else {
                const long long per = (long long)p.Ho * p.Wo;
                const long long b = m / per;
                const int rem = (int)(m - b * per);
                const int ho = rem / p.Wo, wo = rem - ho * p.Wo;
                src[j] = (b * p.H + 2 * ho) * p.W + 2 * wo;
            }
        }
    }
    __device__ __forceinline__ void fetch(const int k0) {
        const int k = k0 + map.sc8 * 8;
        kok = k < p.C;
        if (kok) {
            const float4 a = *(const float4*)(p.s1 + k), b = *(const float4*)(p.s1 + k + 4);
            const float4 c = *(const float4*)(p.h1 + k), d = *(const float4*)(p.h1 + k + 4);
            sv[0] = a.x; sv[1] = a.y; sv[2] = a.z; sv[3] = a.w; sv[4] = b.x; sv[5] = b.y; sv[6] = b.z; sv[7] = b.w;
            hv[0] = c.x; hv[1] = c.y; hv[2] = c.z; hv[3] = c.w; hv[4] = d.x; hv[5] = d.y; hv[6] = d.z; hv[7] = d.w;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (kok && row_ok[j]) {
#pragma unroll
                for (int e = 0; e < P * P; ++e)
                    xr[j][e] = *(const uint4*)(p.x + (src[j] + (e >> 1) * p.W + (e & 1)) * p.ldx + k);
            }
        }
    }
    __device__ __forceinline__ void stash(char* buf) const {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            uint4 o = make_uint4(0, 0, 0, 0);                       // past C / past M: zero AFTER the pre-activation
            if (kok && row_ok[j]) {
                float a[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) a[i] = 0.f;
#pragma unroll
                for (int e = 0; e < P * P; ++e) preact_acc8(a, xr[j][e], sv, hv);
                if (P == 2) {
#pragma unroll
                    for (int i = 0; i < 8; ++i) a[i] *= 0.25f;
                }
                o = make_uint4(pack_bf2(a[0], a[1]), pack_bf2(a[2], a[3]), pack_bf2(a[4], a[5]), pack_bf2(a[6], a[7]));
            }
            map.put(buf, 0, j, o);
        }
    }
};

template <int P>
__global__ __launch_bounds__(PW_THREADS) void preact1x1_kernel(const PreactP p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    f32x16 acc[2][2];
    PreactRows<P> rows{p};
    rows.init();
    pw128_product(acc, smem, rows, p.w, p.C, p.N);
    pw128_epilogue(acc, p.M, p.N, [&](const f32x16& a, const long long m, const int n) {
        bf16_t* dst = p.y + m * p.ldy + p.cy + n;
        if (p.s2) store16_relu(a, p.s2 + n, p.h2 + n, dst);
        else store16_plain(a, dst);
    });
}

}  // namespace

}  // namespace mv

extern "C" {

int mv_preact_conv1x1_supported(int C, int N, int ldx, int ldy, int cy, int pool, int x_dtype, int y_dtype) {
    if (mv::get_flag("no_dense_fused") || mv::get_flag("force_generic")) return 0;
    if (x_dtype != MV_BF16 || y_dtype != MV_BF16) return 0;
    if (pool != 1 && pool != 2) return 0;
    if (C < 16 || C > 8192 || N < 16 || N > 8192 || ldx < C || ldx > (1 << 20) || ldy > (1 << 20)) return 0;
    if ((C | N | ldx | ldy | cy) & 15) return 0;
    if (cy < 0 || cy + N > ldy) return 0;
    return 1;
}

int mv_preact_conv1x1_fwd(const void* x, int ldx, const float* s1, const float* h1, const void* w, const float* s2, const float* h2,
                          void* y, int ldy, int cy, int B, int H, int W, int C, int N, int pool, int x_dtype, int y_dtype,
                          mv_stream_t stream_) {
    using namespace mv;
    MV_CHECK_ARG(x && s1 && h1 && w && y, "mv_preact_conv1x1_fwd: NULL argument");
    MV_CHECK_ARG((s2 == nullptr) == (h2 == nullptr), "mv_preact_conv1x1_fwd: s2 and h2 go together (both NULL: the identity)");
    MV_CHECK_ARG(x != y, "mv_preact_conv1x1_fwd: not in place");
    MV_CHECK_ARG(pool == 1 || pool == 2, "mv_preact_conv1x1_fwd: pool=%d (1 or 2)", pool);
    MV_CHECK_ARG(B >= 1 && H >= pool && W >= pool && H <= 65536 && W <= 65536, "mv_preact_conv1x1_fwd: B=%d H=%d W=%d with pool=%d", B,
                 H, W, pool);
    MV_CHECK_ARG(cy >= 0 && N >= 0 && cy + N <= ldy, "mv_preact_conv1x1_fwd: output slice [%d, +%d) of rows of %d", cy, N, ldy);
    if (!mv_preact_conv1x1_supported(C, N, ldx, ldy, cy, pool, x_dtype, y_dtype)) {
        set_error("mv_preact_conv1x1_fwd: unsupported C=%d N=%d ldx=%d ldy=%d cy=%d pool=%d x_dtype=%d y_dtype=%d (ask "
                  "mv_preact_conv1x1_supported first)", C, N, ldx, ldy, cy, pool, x_dtype, y_dtype);
        return MV_E_UNSUPPORTED;
    }
    PreactP p;
    p.x = (const bf16_t*)x; p.w = (const bf16_t*)w; p.s1 = s1; p.h1 = h1; p.s2 = s2; p.h2 = h2; p.y = (bf16_t*)y;
    p.ldx = ldx; p.ldy = ldy; p.C = C; p.N = N; p.cy = cy; p.H = H; p.W = W; p.Ho = H / pool; p.Wo = W / pool;
    p.M = (long long)B * p.Ho * p.Wo;
    MV_CHECK_ARG((long long)B * H * W < (1ll << 31) - 8192, "mv_preact_conv1x1_fwd: %lld pixels", (long long)B * H * W);
    const dim3 grid((unsigned)((p.M + PW_TM - 1) / PW_TM), (unsigned)((N + PW_TN - 1) / PW_TN));
    hipStream_t st = (hipStream_t)stream_;
    if (pool == 1) {
        static LdsAttrSite site;
        MV_HIP(site.ensure((const void*)preact1x1_kernel<1>, PW_LDS));
        set_kernel_name(s2 ? "preact1x1_relu" : "preact1x1");
        hipLaunchKernelGGL(preact1x1_kernel<1>, grid, dim3(PW_THREADS), PW_LDS, st, p);
    } else {
        static LdsAttrSite site;
        MV_HIP(site.ensure((const void*)preact1x1_kernel<2>, PW_LDS));
        set_kernel_name(s2 ? "preact1x1_pool2_relu" : "preact1x1_pool2");
        hipLaunchKernelGGL(preact1x1_kernel<2>, grid, dim3(PW_THREADS), PW_LDS, st, p);
    }
    MV_LAUNCH_CHECK();
    return MV_OK;
}

}  // extern "C"
