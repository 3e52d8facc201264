// Pointwise convolution with folded BatchNorm + ReLU whose output columns go to ONE or TWO strided destinations (GoogLeNet's
// Inception module, reference googlenet.py:229-237: the merged 1x1 of branch 1 and the two reduce convolutions; the pool projection).
// NHWC bf16, fp32 accumulation on the matrix cores, gfx950.
//
//   v[m, n] = relu( scale[n] * sum_{c<C} w[n][c] x[m][c] + shift[n] )           m < M, n < N
//   n <  n0:  dst0[m * ld0 + c0 + n]        = v[m, n]
//   n >= n0:  dst1[m * ld1 + c1 + (n - n0)] = v[m, n]
//
// so a branch lands in its channel slice of the module's output and nothing is concatenated afterwards.  The tile, the chunk loop and
// the epilogue walk are pw128.h's; the B operand is the dense rows of x as they are, and a lane's 16 consecutive channels go to
// whichever destination the group belongs (n0 is a multiple of 16).
#include "pw128.h"

namespace mv {

namespace {

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

__global__ __launch_bounds__(PW_THREADS) void conv1x1_split_kernel(const SplitP p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    f32x16 acc[2][2];
    PwRowStager rows{p.x, p.M, pw128_m0(), p.C, 0};                  // the B operand: the dense rows of x as they are
    pw128_product(acc, smem, rows, p.w, p.C, p.N);
    pw128_epilogue(acc, p.M, p.N, [&](const f32x16& a, const long long m, const int n) {
        bf16_t* dst = n < p.n0 ? p.dst0 + m * p.ld0 + p.c0 + n : p.dst1 + m * p.ld1 + p.c1 + (n - p.n0);
        store16_relu(a, p.scale + n, p.shift + n, dst);
    });
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
    MV_HIP(site.ensure((const void*)conv1x1_split_kernel, PW_LDS));
    const dim3 grid((unsigned)((M + PW_TM - 1) / PW_TM), (unsigned)((N + PW_TN - 1) / PW_TN));
    set_kernel_name(n0 < N ? "conv1x1_split2" : "conv1x1_split1");
    hipLaunchKernelGGL(conv1x1_split_kernel, grid, dim3(PW_THREADS), PW_LDS, (hipStream_t)stream_, p);
    MV_LAUNCH_CHECK();
    return MV_OK;
}

}  // extern "C"
