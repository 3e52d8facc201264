// DenseNet dense layer, conv2 (reference densenet.py:44-52, 65): a plain 3x3 convolution, padding 1, stride 1, of the bottleneck map t
// into the layer's channel slice of the block's buffer, so nothing is concatenated afterwards.  NO affine step and NO ReLU: the next
// consumers apply their own BatchNorm to these values, negatives included.  NHWC bf16, fp32 accumulation on the matrix cores, gfx950.
//
//   y[m * ldy + cy + n] = sum_{r,s<3, c<S} W[n][c][r][s] t[b, h + r - 1, w + s - 1, c]        n < N, m = b H W + h W + w
//
// inception_pair.hip with one convolution and the identity epilogue: a workgroup stages the flat range of its pixel tile in LDS once
// (flat3x3.h: the range, the zero slot, the fragment order, the k-loop; host: ops.inception_fragments pads the rows to a multiple of
// 32), a wave owns 32 pixels and one pair of 32-channel output tiles (blockIdx.y).  The growth rate is 32 or 48: ONE pair, and at
// N = 48 the upper half of the second tile is computed on zero rows and never stored.  With a single job per pixel tile the pixel
// tile is all there is to fill the machine with, so it comes in two sizes: 128 pixels (4 waves) and 64 pixels (2 waves, half the LDS
// and twice the workgroups for the 14 x 14 and 7 x 7 maps); the host picks by the pixel count.
#include "flat3x3.h"

namespace mv {

namespace {

constexpr int CS3_LDS_MAX = 160 * 1024;
constexpr long long CS3_SMALL_M = 128ll * 1024;      // below this many pixels: the 64-pixel tile

struct SliceP {
    const bf16_t* t;
    bf16_t* y;
    const uint4* wf;       // [ceil(N / 32)][9 S / 16][64] fragments
    long long ldt, ldy, M;
    int H, W, S, N, cy;
    int n_slots;           // TM + 2 W + 2 staged pixels; slot n_slots is the zero pixel
};

template <int NW>
__global__ __launch_bounds__(64 * NW) void conv3x3_slice_kernel(const SliceP p) {
    constexpr int TM = 32 * NW;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long m0 = (long long)blockIdx.x * TM;
    const int W = p.W, KC = p.S >> 4, row_b = 2 * p.S + 16;
    const int tile0 = 2 * (int)blockIdx.y;

    // ---- 1. the flat pixel range of t and the zero pixel to LDS
    flat_stage<64 * NW>(smem, p.t, p.ldt, 0, 2 * KC, m0, W, p.M, p.n_slots, row_b, tid);

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
    const int tiles = (p.N + 31) >> 5;
    const uint4* wt = p.wf + (long long)tile0 * (9 * KC) * 64;
    if (tile0 + 1 < tiles) flat_taps9<2>(wt, smem, off, acc, KC, lane);
    else flat_taps9<1>(wt, smem, off, acc, KC, lane);
    if (m >= p.M) return;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int n = (tile0 + j) * 32 + 16 * hh;                   // first of the lane's 16 channels
        if (n + 16 <= p.N) store16_plain(acc[j], p.y + m * p.ldy + p.cy + n);
    }
}

template <int NW>
int slice_go(SliceP p, hipStream_t st) {
    constexpr int TM = 32 * NW;
    static LdsAttrSite site;
    auto kern = conv3x3_slice_kernel<NW>;
    p.n_slots = TM + 2 * p.W + 2;
    const size_t smem = flat_lds_bytes(TM, p.W, p.S);
    MV_HIP(site.ensure((const void*)kern, smem));
    const dim3 grid((unsigned)((p.M + TM - 1) / TM), (unsigned)(((p.N + 31) / 32 + 1) / 2));
    hipLaunchKernelGGL(kern, grid, dim3(64 * NW), smem, st, p);
    MV_LAUNCH_CHECK();
    return MV_OK;
}

}  // namespace

}  // namespace mv

extern "C" {

int mv_conv3x3_slice_supported(int S, int N, int H, int W, int x_dtype, int y_dtype) {
    if (mv::get_flag("no_dense_fused") || mv::get_flag("force_generic")) return 0;
    if (x_dtype != MV_BF16 || y_dtype != MV_BF16) return 0;
    if (S < 16 || S > 512 || N < 16 || N > 4096 || ((S | N) & 15)) return 0;
    if (H < 1 || W < 1 || H > 4096 || W > 4096) return 0;
    return mv::flat_lds_bytes(128, W, S) <= (size_t)mv::CS3_LDS_MAX;          // the tile and its halo rows have to fit LDS
}

int mv_conv3x3_slice_fwd(const void* t, int ldt, int S, const void* w_frag, void* y, int ldy, int cy, int N, int B, int H, int W,
                         int x_dtype, int y_dtype, mv_stream_t stream_) {
    using namespace mv;
    MV_CHECK_ARG(t && w_frag && y, "mv_conv3x3_slice_fwd: NULL argument");
    MV_CHECK_ARG(t != y, "mv_conv3x3_slice_fwd: not in place");
    MV_CHECK_ARG(B >= 1, "mv_conv3x3_slice_fwd: B=%d", B);
    if (!mv_conv3x3_slice_supported(S, N, H, W, x_dtype, y_dtype)) {
        set_error("mv_conv3x3_slice_fwd: unsupported S=%d N=%d H=%d W=%d x_dtype=%d y_dtype=%d (ask mv_conv3x3_slice_supported first)", S,
                  N, H, W, x_dtype, y_dtype);
        return MV_E_UNSUPPORTED;
    }
    MV_CHECK_ARG(!((ldt | ldy | cy) & 15) && cy >= 0, "mv_conv3x3_slice_fwd: strides and offsets are non-negative multiples of 16 "
                 "(ldt=%d ldy=%d cy=%d)", ldt, ldy, cy);
    MV_CHECK_ARG(S <= ldt, "mv_conv3x3_slice_fwd: %d channels of rows of %d", S, ldt);
    MV_CHECK_ARG(cy + N <= ldy, "mv_conv3x3_slice_fwd: output slice [%d, +%d) of rows of %d", cy, N, ldy);
    SliceP p;
    p.t = (const bf16_t*)t; p.y = (bf16_t*)y; p.wf = (const uint4*)w_frag; p.ldt = ldt; p.ldy = ldy;
    p.M = (long long)B * H * W;
    MV_CHECK_ARG(p.M < (1ll << 31) - 8192, "mv_conv3x3_slice_fwd: %lld pixels", p.M);
    p.H = H; p.W = W; p.S = S; p.N = N; p.cy = cy; p.n_slots = 0;
    // flags "dense3x3_m64" / "dense3x3_m128": that tile whatever the pixel count (measurements, and the parity tests run both)
    const bool small = !get_flag("dense3x3_m128") && (p.M < CS3_SMALL_M || get_flag("dense3x3_m64"));
    set_kernel_name(small ? "conv3x3_slice_m64" : "conv3x3_slice_m128");
    return small ? slice_go<2>(p, (hipStream_t)stream_) : slice_go<4>(p, (hipStream_t)stream_);
}

}  // extern "C"
