// Pointwise convolution with folded BatchNorm + ReLU whose output columns go to ONE or TWO strided destinations (GoogLeNet's
// Inception module, reference googlenet.py:229-237: the merged 1x1 of branch 1 and the two reduce convolutions; the pool projection).
// NHWC bf16, fp32 accumulation on the matrix cores, gfx950.
//
//   v[m, n] = relu( scale[n] * sum_{c<C} w[n][c] x[m][c] + shift[n] )           m < M, n < N
//   n <  n0:  dst0[m * ld0 + c0 + n]        = v[m, n]
//   n >= n0:  dst1[m * ld1 + c1 + (n - n0)] = v[m, n]
//
// so a branch lands in its channel slice of the module's output and nothing is concatenated afterwards.  A 256-thread workgroup owns
// 128 rows x 128 columns; the four waves are a 2 x 2 grid of 64 x 64 sub-tiles on v_mfma_f32_32x32x16_bf16 with the weights as the A
// operand (rows = output channels) and the pixels as the B operand.  The reduction runs in chunks of 64 channels: both operands of a
// chunk are staged in LDS (rows of 128 + 16 bytes: the 16-byte reads of 32 consecutive rows fall on different bank quads), double
// buffered, with the next chunk's global loads in flight in registers while the matrix cores work on the current one -- one barrier
// per chunk.  The lane reads weight row mfma32_tile_row(lane % 32) of its 32-row tile, so its 16 accumulator registers are 16
// CONSECUTIVE output channels of one pixel (flat3x3.h): scale, shift, ReLU and two 16-byte stores, to whichever destination the
// 16-channel group belongs (n0 is a multiple of 16).  Rows past M, columns past N and channels past C are zeros in
// LDS and are never read from memory.
#include "flat3x3.h"

namespace mv {

namespace {

constexpr int CS_THREADS = 256;
constexpr int CS_TM = 128, CS_TN = 128, CS_KC = 64;
constexpr int CS_ROW_B = 2 * CS_KC + 16;
constexpr int CS_BUF_B = (CS_TM + CS_TN) * CS_ROW_B;
constexpr int CS_LDS = 2 * CS_BUF_B;

struct SplitP {
    const bf16_t* x;       // [M][C]
    const bf16_t* w;       // [N][C]
    const float* scale;    // [N]
    const float* shift;    // [N]
    bf16_t* dst0;
    bf16_t* dst1;          // null when n0 == N
    long long M, ld0, ld1;
    int C, N, n0, c0, c1;
};

__global__ __launch_bounds__(CS_THREADS) void conv1x1_split_kernel(const SplitP p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long m0 = (long long)blockIdx.x * CS_TM;
    const int nb0 = blockIdx.y * CS_TN;
    const int wm = wave & 1, wn = wave >> 1;
    const int hh = lane >> 5, pl = lane & 31;
    const int chan = mfma32_tile_row(pl);

    // staging: the thread moves 16-byte piece tid % 8 of rows tid / 8 + 32 j of both operands
    const int sr = tid >> 3, sc8 = tid & 7;
    uint4 xr[4], wr[4];
    auto fetch = [&](const int k0) {
        const int k = k0 + sc8 * 8;
        const bool kok = k < p.C;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long long m = m0 + sr + 32 * j;
            const int n = nb0 + sr + 32 * j;
            xr[j] = make_uint4(0, 0, 0, 0);
            wr[j] = make_uint4(0, 0, 0, 0);
            if (kok && m < p.M) xr[j] = *(const uint4*)(p.x + m * p.C + k);
            if (kok && n < p.N) wr[j] = *(const uint4*)(p.w + (long long)n * p.C + k);
        }
    };
    auto stash = [&](char* buf) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            *(uint4*)(buf + (sr + 32 * j) * CS_ROW_B + sc8 * 16) = xr[j];
            *(uint4*)(buf + (CS_TM + sr + 32 * j) * CS_ROW_B + sc8 * 16) = wr[j];
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
    const int a_off = (CS_TM + wn * 64 + chan) * CS_ROW_B + hh * 16;
    const int b_off = (wm * 64 + pl) * CS_ROW_B + hh * 16;
    const int nchunks = (p.C + CS_KC - 1) / CS_KC;
    fetch(0);
    stash(smem);
    __syncthreads();
    for (int ch = 0; ch < nchunks; ++ch) {
        const char* cur = smem + (ch & 1) * CS_BUF_B;
        const bool more = ch + 1 < nchunks;
        if (more) fetch((ch + 1) * CS_KC);
        if (wave_live) {
            const int left = (p.C - ch * CS_KC) >> 4;
            const int nks = left < 4 ? left : 4;
            for (int ks = 0; ks < nks; ++ks) {
                const bf16x8 a0 = __builtin_bit_cast(bf16x8, *(const uint4*)(cur + a_off + ks * 32));
                const bf16x8 a1 = __builtin_bit_cast(bf16x8, *(const uint4*)(cur + a_off + 32 * CS_ROW_B + ks * 32));
                const bf16x8 b0 = __builtin_bit_cast(bf16x8, *(const uint4*)(cur + b_off + ks * 32));
                const bf16x8 b1 = __builtin_bit_cast(bf16x8, *(const uint4*)(cur + b_off + 32 * CS_ROW_B + ks * 32));
                acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b0, acc[0][0], 0, 0, 0);
                acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b0, acc[1][0], 0, 0, 0);
                acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b1, acc[0][1], 0, 0, 0);
                acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b1, acc[1][1], 0, 0, 0);
            }
        }
        if (more) stash(smem + ((ch + 1) & 1) * CS_BUF_B);          // the other buffer: every wave left it before the last barrier
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
            bf16_t* dst = n < p.n0 ? p.dst0 + m * p.ld0 + p.c0 + n : p.dst1 + m * p.ld1 + p.c1 + (n - p.n0);
            store16_relu(acc[j][q], p.scale + n, p.shift + n, dst);
        }
    }
}

}  // namespace

}  // namespace mv

extern "C" {

int mv_conv1x1_split_supported(int C, int N, int n0, int ld0, int c0, int ld1, int c1, int x_dtype, int y_dtype) {
    if (mv::get_flag("no_inception_fused") || mv::get_flag("force_generic")) return 0;
    if (x_dtype != MV_BF16 || y_dtype != MV_BF16) return 0;
    if (C < 16 || C > 8192 || N < 16 || N > 8192 || n0 < 16 || n0 > N) return 0;
    if ((C | N | n0 | ld0 | c0) & 15) return 0;
    if (c0 < 0 || c0 + n0 > ld0) return 0;
    if (n0 < N) {
        if ((ld1 | c1) & 15) return 0;
        if (c1 < 0 || c1 + (N - n0) > ld1) return 0;
    }
    return 1;
}

int mv_conv1x1_split_fwd(const void* x, const void* w, const float* scale, const float* shift, void* dst0, int ld0, int c0, void* dst1,
                         int ld1, int c1, int64_t M, int C, int N, int n0, int x_dtype, int y_dtype, mv_stream_t stream_) {
    using namespace mv;
    MV_CHECK_ARG(x && w && scale && shift && dst0, "mv_conv1x1_split_fwd: NULL argument");
    MV_CHECK_ARG(x != dst0 && x != dst1, "mv_conv1x1_split_fwd: not in place");
    MV_CHECK_ARG(M >= 1 && M < (1ll << 31) - 8192, "mv_conv1x1_split_fwd: M=%lld", (long long)M);
    MV_CHECK_ARG((n0 == N) == (dst1 == nullptr), "mv_conv1x1_split_fwd: dst1 goes with n0 < N (n0=%d N=%d)", n0, N);
    if (!mv_conv1x1_split_supported(C, N, n0, ld0, c0, ld1, c1, x_dtype, y_dtype)) {
        set_error("mv_conv1x1_split_fwd: unsupported C=%d N=%d n0=%d ld0=%d c0=%d ld1=%d c1=%d x_dtype=%d y_dtype=%d (ask "
                  "mv_conv1x1_split_supported first)", C, N, n0, ld0, c0, ld1, c1, x_dtype, y_dtype);
        return MV_E_UNSUPPORTED;
    }
    SplitP p;
    p.x = (const bf16_t*)x; p.w = (const bf16_t*)w; p.scale = scale; p.shift = shift;
    p.dst0 = (bf16_t*)dst0; p.dst1 = (bf16_t*)dst1;
    p.M = M; p.ld0 = ld0; p.ld1 = ld1; p.C = C; p.N = N; p.n0 = n0; p.c0 = c0; p.c1 = c1;
    static LdsAttrSite site;
    MV_HIP(site.ensure((const void*)conv1x1_split_kernel, CS_LDS));
    const dim3 grid((unsigned)((M + CS_TM - 1) / CS_TM), (unsigned)((N + CS_TN - 1) / CS_TN));
    set_kernel_name(n0 < N ? "conv1x1_split2" : "conv1x1_split1");
    hipLaunchKernelGGL(conv1x1_split_kernel, grid, dim3(CS_THREADS), CS_LDS, (hipStream_t)stream_, p);
    MV_LAUNCH_CHECK();
    return MV_OK;
}

}  // extern "C"
