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
// that a later layer has not written yet.  The tile is conv1x1_split.hip's: a 256-thread workgroup owns 128 output pixels x 128 output
// channels, four waves as a 2 x 2 grid of 64 x 64 sub-tiles on v_mfma_f32_32x32x16_bf16, weights as the A operand, 64-channel chunks
// of both operands in LDS (rows of 128 + 16 bytes), double buffered, the next chunk's global loads in flight in registers while the
// matrix cores work -- the affine step, the ReLU, the mean and the rounding happen when those registers are written to LDS, behind
// the chunk's MFMAs.  Reduction channels past C and rows past M must be ZERO AFTER the pre-activation, and relu(0 * s + h) is not
// zero: they are masked behind the affine step (zeros are written to LDS) and are never loaded.  The lane reads weight row
// mfma32_tile_row(lane % 32), so its 16 accumulator registers are 16 consecutive output channels (flat3x3.h: store16_relu /
// store16_plain).
#include "flat3x3.h"

namespace mv {

namespace {

constexpr int PA_THREADS = 256;
constexpr int PA_TM = 128, PA_TN = 128, PA_KC = 64;
constexpr int PA_ROW_B = 2 * PA_KC + 16;
constexpr int PA_BUF_B = (PA_TM + PA_TN) * PA_ROW_B;
constexpr int PA_LDS = 2 * PA_BUF_B;

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

template <int P>
__global__ __launch_bounds__(PA_THREADS) void preact1x1_kernel(const PreactP p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long m0 = (long long)blockIdx.x * PA_TM;
    const int nb0 = blockIdx.y * PA_TN;
    const int wm = wave & 1, wn = wave >> 1;
    const int hh = lane >> 5, pl = lane & 31;
    const int chan = mfma32_tile_row(pl);

    // staging: the thread moves 16-byte piece tid % 8 of rows tid / 8 + 32 j of both operands; a pixel row of the B operand is made
    // of the P x P source pixels src[j] + {0, 1} + {0, W}
    const int sr = tid >> 3, sc8 = tid & 7;
    long long src[4];
    bool row_ok[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const long long m = m0 + sr + 32 * j;
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
    uint4 xr[4][P * P], wr[4];
    float sv[8], hv[8];
    bool kok = false;
    auto fetch = [&](const int k0) {
        const int k = k0 + sc8 * 8;
        kok = k < p.C;
        if (kok) {
            const float4 a = *(const float4*)(p.s1 + k), b = *(const float4*)(p.s1 + k + 4);
            const float4 c = *(const float4*)(p.h1 + k), d = *(const float4*)(p.h1 + k + 4);
            sv[0] = a.x; sv[1] = a.y; sv[2] = a.z; sv[3] = a.w; sv[4] = b.x; sv[5] = b.y; sv[6] = b.z; sv[7] = b.w;
            hv[0] = c.x; hv[1] = c.y; hv[2] = c.z; hv[3] = c.w; hv[4] = d.x; hv[5] = d.y; hv[6] = d.z; hv[7] = d.w;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int n = nb0 + sr + 32 * j;
            wr[j] = make_uint4(0, 0, 0, 0);
            if (kok && n < p.N) wr[j] = *(const uint4*)(p.w + (long long)n * p.C + k);
            if (kok && row_ok[j]) {
#pragma unroll
                for (int e = 0; e < P * P; ++e)
                    xr[j][e] = *(const uint4*)(p.x + (src[j] + (e >> 1) * p.W + (e & 1)) * p.ldx + k);
            }
        }
    };
    auto stash = [&](char* buf) {
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
            *(uint4*)(buf + (sr + 32 * j) * PA_ROW_B + sc8 * 16) = o;
            *(uint4*)(buf + (PA_TM + sr + 32 * j) * PA_ROW_B + sc8 * 16) = wr[j];
        }
    };

    f32x16 acc[2][2];                                               // [channel tile j][pixel tile q]
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[j][q][e] = 0.f;

    const bool wave_live = nb0 + wn * 64 < p.N;                     // a wave whose 64 columns are all past N only stages
    const int a_off = (PA_TM + wn * 64 + chan) * PA_ROW_B + hh * 16;
    const int b_off = (wm * 64 + pl) * PA_ROW_B + hh * 16;
    const int nchunks = (p.C + PA_KC - 1) / PA_KC;
    fetch(0);
    stash(smem);
    __syncthreads();
    for (int ch = 0; ch < nchunks; ++ch) {
        const char* cur = smem + (ch & 1) * PA_BUF_B;
        const bool more = ch + 1 < nchunks;
        if (more) fetch((ch + 1) * PA_KC);
        if (wave_live) {
            const int left = (p.C - ch * PA_KC) >> 4;
            const int nks = left < 4 ? left : 4;
            for (int ks = 0; ks < nks; ++ks) {
                const bf16x8 a0 = __builtin_bit_cast(bf16x8, *(const uint4*)(cur + a_off + ks * 32));
                const bf16x8 a1 = __builtin_bit_cast(bf16x8, *(const uint4*)(cur + a_off + 32 * PA_ROW_B + ks * 32));
                const bf16x8 b0 = __builtin_bit_cast(bf16x8, *(const uint4*)(cur + b_off + ks * 32));
                const bf16x8 b1 = __builtin_bit_cast(bf16x8, *(const uint4*)(cur + b_off + 32 * PA_ROW_B + ks * 32));
                acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b0, acc[0][0], 0, 0, 0);
                acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b0, acc[1][0], 0, 0, 0);
                acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b1, acc[0][1], 0, 0, 0);
                acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b1, acc[1][1], 0, 0, 0);
            }
        }
        if (more) stash(smem + ((ch + 1) & 1) * PA_BUF_B);          // the other buffer: every wave left it before the last barrier
        __syncthreads();
    }

    if (!wave_live) return;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int n = nb0 + wn * 64 + j * 32 + 16 * hh;             // first of the lane's 16 columns
        if (n >= p.N) continue;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const long long m = m0 + wm * 64 + q * 32 + pl;
            if (m >= p.M) continue;
            bf16_t* dst = p.y + m * p.ldy + p.cy + n;
            if (p.s2) store16_relu(acc[j][q], p.s2 + n, p.h2 + n, dst);
            else store16_plain(acc[j][q], dst);
        }
    }
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
    const dim3 grid((unsigned)((p.M + PA_TM - 1) / PA_TM), (unsigned)((N + PA_TN - 1) / PA_TN));
    hipStream_t st = (hipStream_t)stream_;
    if (pool == 1) {
        static LdsAttrSite site;
        MV_HIP(site.ensure((const void*)preact1x1_kernel<1>, PA_LDS));
        set_kernel_name(s2 ? "preact1x1_relu" : "preact1x1");
        hipLaunchKernelGGL(preact1x1_kernel<1>, grid, dim3(PA_THREADS), PA_LDS, st, p);
    } else {
        static LdsAttrSite site;
        MV_HIP(site.ensure((const void*)preact1x1_kernel<2>, PA_LDS));
        set_kernel_name(s2 ? "preact1x1_pool2_relu" : "preact1x1_pool2");
        hipLaunchKernelGGL(preact1x1_kernel<2>, grid, dim3(PA_THREADS), PA_LDS, st, p);
    }
    MV_LAUNCH_CHECK();
    return MV_OK;
}

}  // extern "C"
