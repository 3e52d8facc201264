// GoogLeNet Inception module, the two 3x3 convolutions of branches 2 and 3 (reference googlenet.py:206-220, 229-237) in ONE launch:
// 3x3, padding 1, stride 1, folded BatchNorm + ReLU each; each reads its channel slice of the reduce map t and writes its channel slice
// of the module's output y, so nothing is concatenated afterwards.  NHWC bf16, fp32 accumulation on the matrix cores, gfx950.
//
//   y[m, cy_i + n] = relu( scale_i[n] * sum_{r,s<3, c<S_i} W_i[n][c][r][s] t[b, h + r - 1, w + s - 1, ct_i + c] + shift_i[n] )   n < N_i
//
// for i = 0, 1; rows of t are ldt apart, rows of y ldy.  A 256-thread workgroup owns 128 consecutive flattened pixels and ONE pair of
// 32-channel output tiles of ONE of the two convolutions (blockIdx.y): 7 x 7 and 14 x 14 maps at batch size are few pixel tiles, the
// output channels fill the machine.  It stages the flat range of its convolution's slice of t (S_i channels per slot) in LDS once
// (flat3x3.h: the range, the zero slot, the fragment order; host: ops.inception_fragments pads the output rows with zeros to a
// multiple of 32).  A wave owns 32 pixels and both tiles of the pair.  N_i is a multiple of 16: the upper half of the last tile may
// not exist (it is computed on the zero rows and not stored), and an odd tile count leaves the last workgroup column a single tile.
#include "flat3x3.h"

namespace mv {

namespace {

constexpr int IP_THREADS = 256;
constexpr int IP_TM = 128;
constexpr int IP_LDS_MAX = 160 * 1024;

struct PairP {
    const bf16_t* t;
    bf16_t* y;
    long long ldt, ldy, M;
    const uint4* wf0; const float* scale0; const float* shift0;      // [ceil(N0 / 32)][9 S0 / 16][64] fragments
    const uint4* wf1; const float* scale1; const float* shift1;
    int H, W;
    int ct0, S0, cy0, N0;
    int ct1, S1, cy1, N1;
    int jobs0;             // blockIdx.y < jobs0: convolution 0, tile pair blockIdx.y; else convolution 1, pair blockIdx.y - jobs0
    int n_slots;           // 128 + 2 W + 2 staged pixels; slot n_slots is the zero pixel
};

__global__ __launch_bounds__(IP_THREADS) void conv3x3_pair_kernel(const PairP p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long m0 = (long long)blockIdx.x * IP_TM;
    const int W = p.W;
    const bool second = (int)blockIdx.y >= p.jobs0;
    const int S = second ? p.S1 : p.S0, N = second ? p.N1 : p.N0;
    const int ct = second ? p.ct1 : p.ct0, cy = second ? p.cy1 : p.cy0;
    const uint4* wf = second ? p.wf1 : p.wf0;
    const float* scale = second ? p.scale1 : p.scale0;
    const float* shift = second ? p.shift1 : p.shift0;
    const int tile0 = 2 * ((int)blockIdx.y - (second ? p.jobs0 : 0));
    const int KC = S >> 4, row_b = 2 * S + 16;

    // ---- 1. the flat pixel range of this convolution's slice of t and the zero pixel to LDS
    flat_stage<IP_THREADS>(smem, p.t, p.ldt, ct, 2 * KC, m0, W, p.M, p.n_slots, row_b, tid);

    // ---- 2. the LDS byte offsets of the nine taps of this lane's pixel
    int off[9];
    const int hh = lane >> 5;
    const int local = wave * 32 + (lane & 31);
    const long long m = m0 + local;
    flat_tap_offsets(off, local, m0, p.M, p.H, W, p.n_slots, row_b, hh);
    __syncthreads();

    // ---- 3. the pair of tiles (one tile where the count is odd)
    f32x16 acc[2];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[j][e] = 0.f;
    const int tiles = (N + 31) >> 5;
    const bool two = tile0 + 1 < tiles;
    const uint4* wt = wf + (long long)tile0 * (9 * KC) * 64;
    if (two) flat_taps9<2>(wt, smem, off, acc, KC, lane);
    else flat_taps9<1>(wt, smem, off, acc, KC, lane);
    if (m >= p.M) return;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int n = (tile0 + j) * 32 + 16 * hh;                   // first of the lane's 16 channels inside its convolution
        if (n + 16 <= N) store16_relu(acc[j], scale + n, shift + n, p.y + m * p.ldy + cy + n);
    }
}

}  // namespace

}  // namespace mv

extern "C" {

int mv_conv3x3_pair_supported(int S0, int S1, int N0, int N1, int H, int W, int x_dtype, int y_dtype) {
    if (mv::get_flag("no_inception_fused") || mv::get_flag("force_generic")) return 0;
    if (x_dtype != MV_BF16 || y_dtype != MV_BF16) return 0;
    if (S0 < 16 || S1 < 16 || S0 > 512 || S1 > 512 || N0 < 16 || N1 < 16 || N0 > 4096 || N1 > 4096) return 0;
    if ((S0 | S1 | N0 | N1) & 15) return 0;
    if (H < 1 || W < 1 || H > 4096 || W > 4096) return 0;
    return mv::flat_lds_bytes(mv::IP_TM, W, S0 > S1 ? S0 : S1) <= (size_t)mv::IP_LDS_MAX;      // the tile and its halo rows have to fit LDS
}

int mv_conv3x3_pair_fwd(const void* t, int ldt, int ct0, int S0, int ct1, int S1, const void* w0_frag, const float* scale0,
                        const float* shift0, const void* w1_frag, const float* scale1, const float* shift1, void* y, int ldy, int cy0,
                        int N0, int cy1, int N1, int B, int H, int W, int x_dtype, int y_dtype, mv_stream_t stream_) {
    using namespace mv;
    MV_CHECK_ARG(t && w0_frag && scale0 && shift0 && w1_frag && scale1 && shift1 && y, "mv_conv3x3_pair_fwd: NULL argument");
    MV_CHECK_ARG(t != y, "mv_conv3x3_pair_fwd: not in place");
    MV_CHECK_ARG(B >= 1, "mv_conv3x3_pair_fwd: B=%d", B);
    if (!mv_conv3x3_pair_supported(S0, S1, N0, N1, H, W, x_dtype, y_dtype)) {
        set_error("mv_conv3x3_pair_fwd: unsupported S0=%d S1=%d N0=%d N1=%d H=%d W=%d x_dtype=%d y_dtype=%d (ask "
                  "mv_conv3x3_pair_supported first)", S0, S1, N0, N1, H, W, x_dtype, y_dtype);
        return MV_E_UNSUPPORTED;
    }
    MV_CHECK_ARG(!((ldt | ct0 | ct1 | ldy | cy0 | cy1) & 15) && ct0 >= 0 && ct1 >= 0 && cy0 >= 0 && cy1 >= 0,
                 "mv_conv3x3_pair_fwd: strides and offsets are non-negative multiples of 16 (ldt=%d ct0=%d ct1=%d ldy=%d cy0=%d cy1=%d)",
                 ldt, ct0, ct1, ldy, cy0, cy1);
    MV_CHECK_ARG(ct0 + S0 <= ldt && ct1 + S1 <= ldt, "mv_conv3x3_pair_fwd: slices [%d, +%d) / [%d, +%d) of rows of %d", ct0, S0, ct1, S1,
                 ldt);
    MV_CHECK_ARG(cy0 + N0 <= ldy && cy1 + N1 <= ldy && (cy0 + N0 <= cy1 || cy1 + N1 <= cy0),
                 "mv_conv3x3_pair_fwd: output slices [%d, +%d) / [%d, +%d) of rows of %d", cy0, N0, cy1, N1, ldy);
    PairP p;
    p.t = (const bf16_t*)t; p.y = (bf16_t*)y; p.ldt = ldt; p.ldy = ldy;
    p.M = (long long)B * H * W;
    MV_CHECK_ARG(p.M < (1ll << 31) - 8192, "mv_conv3x3_pair_fwd: %lld pixels", p.M);
    p.wf0 = (const uint4*)w0_frag; p.scale0 = scale0; p.shift0 = shift0;
    p.wf1 = (const uint4*)w1_frag; p.scale1 = scale1; p.shift1 = shift1;
    p.H = H; p.W = W;
    p.ct0 = ct0; p.S0 = S0; p.cy0 = cy0; p.N0 = N0;
    p.ct1 = ct1; p.S1 = S1; p.cy1 = cy1; p.N1 = N1;
    const int tiles0 = (N0 + 31) / 32, tiles1 = (N1 + 31) / 32;
    p.jobs0 = (tiles0 + 1) / 2;
    const int jobs = p.jobs0 + (tiles1 + 1) / 2;
    p.n_slots = IP_TM + 2 * W + 2;
    const size_t smem = flat_lds_bytes(IP_TM, W, S0 > S1 ? S0 : S1);
    static LdsAttrSite site;
    MV_HIP(site.ensure((const void*)conv3x3_pair_kernel, smem));
    const dim3 grid((unsigned)((p.M + IP_TM - 1) / IP_TM), (unsigned)jobs);
    set_kernel_name("conv3x3_pair");
    hipLaunchKernelGGL(conv3x3_pair_kernel, grid, dim3(IP_THREADS), smem, (hipStream_t)stream_, p);
    MV_LAUNCH_CHECK();
    return MV_OK;
}

}  // extern "C"
