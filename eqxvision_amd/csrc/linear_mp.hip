// Mixed-precision Linear for the training step: forward, input gradient and weight gradient with bf16 operands and fp32
// accumulation on v_mfma_f32_32x32x16_bf16.  All tensors are fp32 in memory; every operand element is rounded to bf16
// (round-to-nearest-even, v_cvt_pk_bf16_f32) on its way into LDS, the result is stored as fp32.
//
// One kernel, C[I,J] = sum over r of A(i,r) B(j,r), with the orientation of each operand in memory as a template parameter:
//   row-major ("RED contiguous")   A is [I][R]: the reduction runs along the contiguous axis
//   transposed ("RED along rows")  A is [R][I]: the reduction runs along the row axis
//     fwd    y [M,N] = x[M,K] . w[N,K]^T    A = x  contiguous, B = w  contiguous, R = K
//     dgrad  dx[M,K] = g[M,N] . w[N,K]      A = g  contiguous, B = w  along rows, R = N
//     wgrad  dw[N,K] = g[M,N]^T . x[M,K]    A = g  along rows, B = x  along rows, R = M
// Neither gradient needs a transposed copy in HBM: an operand whose reduction runs along its rows is staged in LDS as it lies in
// memory ([32 reduction rows][128 columns]) and its MFMA fragment is gathered with ds_read_b64_tr_b16, the transposed LDS read.
//
// Tile: 128 x 128 outputs per workgroup of 4 waves (64 x 64 per wave = 2 x 2 MFMA tiles), 32 reduction elements per step, LDS
// double-buffered with the next step's global loads in flight in registers (one barrier per step).
//
// The LDS images, the staging helpers, the fragment reads, the MFMA step, that loop (lmp_reduce), the store of a tile and the weight
// gradient's split rule are linear_mp_tile.h (shared with conv_mp.hip); the parts of a split are taken from the scratch offer by
// take_scratch_parts (runtime.hip) and added by sum_parts (train_bwd.hip).  Here: the tile decoding, the reduction range, the loaders.
//
// Bounds: rows / columns / reduction elements outside the tensors are never read -- their buffer offset is BUF_OOB, which the buffer
// unit answers with zeros (mfma_common.h) -- and contribute exact zeros to the sums; stores are predicated.  16-byte loads are used
// when the operand's base and row pitch are 16-byte aligned, four guarded 4-byte loads per chunk otherwise.
#include "linear_mp_tile.h"

namespace mv {
namespace {

struct LmpP {
    const float* a;
    const float* b;
    const float* bias;       // [J] or null, added in fp32
    float* c;                // [I][J], or the parts [gridDim.y][I][J] of a split reduction
    long long I, R;          // output rows, reduction length
    int J;                   // output columns
    long long lda, ldb;      // row pitch of each operand in elements
    int vec_a, vec_b;        // 16-byte loads allowed
    long long chunk;         // reduction elements per part (a multiple of LMP_S; >= R when not split)
    int tiles_j;
};

template <bool TA, bool TB> __global__ __launch_bounds__(256) void lmp_kernel(const LmpP p) {
    __shared__ __attribute__((aligned(16))) char lds[2][2][LMP_IMG];
    const int t = threadIdx.x;
    const long long tile_i = blockIdx.x / p.tiles_j;
    const int tile_j = (int)(blockIdx.x - tile_i * p.tiles_j);
    const long long i0 = tile_i * LMP_T;
    const int j0 = tile_j * LMP_T;
    const long long rbeg = (long long)blockIdx.y * p.chunk;
    const long long rend = rbeg + p.chunk < p.R ? rbeg + p.chunk : p.R;
    const int steps = (int)((rend - rbeg + LMP_S - 1) / LMP_S);
    const int rows_a = (int)(p.I - i0 < LMP_T ? p.I - i0 : LMP_T), rows_b = p.J - j0 < LMP_T ? p.J - j0 : LMP_T;
    // contiguous operands: one descriptor at the tile's first row, the reduction offset stays below 2^31 bytes (the host checks the pitch)
    // row-axis operands: the descriptor moves with the reduction row (64-bit), so that offsets stay small for any M
    const float* abase = TA ? p.a + i0 : p.a + i0 * p.lda;
    const float* bbase = TB ? p.b + j0 : p.b + (long long)j0 * p.ldb;

    long long r0 = rbeg;                     // first reduction element of the step the next load stages
    f32x16 acc[2][2];
    lmp_reduce<TA, TB>(acc, lds, steps, t, [&](float4 (&va)[4], float4 (&vb)[4]) {
        const int left = (int)(rend - r0 < LMP_S ? rend - r0 : LMP_S);
        if (TA) lmp_gload<true>(va, abase + r0 * p.lda, p.lda, p.vec_a, rows_a, 0, left, t);
        else    lmp_gload<false>(va, abase, p.lda, p.vec_a, rows_a, (int)r0, left, t);
        if (TB) lmp_gload<true>(vb, bbase + r0 * p.ldb, p.ldb, p.vec_b, rows_b, 0, left, t);
        else    lmp_gload<false>(vb, bbase, p.ldb, p.vec_b, rows_b, (int)r0, left, t);
        r0 += LMP_S;
    });
    // part blockIdx.y of a split reduction, the tile's first row (64-bit: I is not bounded)
    lmp_store_tile(acc, p.c + ((long long)blockIdx.y * p.I + i0) * p.J, (unsigned)p.J, rows_a, j0, p.J, p.bias, t);
}

template <bool TA, bool TB> int lmp_launch(LmpP& p, int split, hipStream_t st) {
    const long long tiles_i = (p.I + LMP_T - 1) / LMP_T;
    p.tiles_j = (p.J + LMP_T - 1) / LMP_T;
    const long long tiles = tiles_i * p.tiles_j;
    if (tiles >= (1LL << 31)) {
        set_error("linear_mp: %lld output tiles do not fit the grid", tiles);
        return MV_E_UNSUPPORTED;
    }
    hipLaunchKernelGGL((lmp_kernel<TA, TB>), dim3((unsigned)tiles, (unsigned)split), dim3(256), 0, st, p);
    return MV_OK;
}

}  // namespace
}  // namespace mv

extern "C" {

using namespace mv;

int mv_linear_mp_fwd(const float* x, const float* w, const float* bias, float* y, int64_t M, int N, int K, mv_stream_t stream) {
    MV_CHECK_ARG(x && w && y && M > 0 && N > 0 && K > 0, "linear_mp_fwd: bad arguments");
    MV_CHECK_ARG(N <= LMP_MAX_DIM && K <= LMP_MAX_DIM, "linear_mp_fwd: N = %d / K = %d above %d", N, K, LMP_MAX_DIM);
    LmpP p = {x, w, bias, y, (long long)M, (long long)K, N, (long long)K, (long long)K, lmp_vec_ok(x, K), lmp_vec_ok(w, K),
              ((long long)K + LMP_S - 1) / LMP_S * LMP_S, 0};
    set_kernel_name("linear_mp_fwd_bf16");
    const int rc = lmp_launch<false, false>(p, 1, (hipStream_t)stream);
    if (rc != MV_OK) return rc;
    MV_LAUNCH_CHECK();
    return MV_OK;
}

int mv_linear_mp_dgrad(const float* g, const float* w, float* dx, int64_t M, int N, int K, mv_stream_t stream) {
    MV_CHECK_ARG(g && w && dx && M > 0 && N > 0 && K > 0, "linear_mp_dgrad: bad arguments");
    MV_CHECK_ARG(N <= LMP_MAX_DIM && K <= LMP_MAX_DIM, "linear_mp_dgrad: N = %d / K = %d above %d", N, K, LMP_MAX_DIM);
    LmpP p = {g, w, nullptr, dx, (long long)M, (long long)N, K, (long long)N, (long long)K, lmp_vec_ok(g, N), lmp_vec_ok(w, K),
              ((long long)N + LMP_S - 1) / LMP_S * LMP_S, 0};
    set_kernel_name("linear_mp_dgrad_bf16");
    const int rc = lmp_launch<false, true>(p, 1, (hipStream_t)stream);
    if (rc != MV_OK) return rc;
    MV_LAUNCH_CHECK();
    return MV_OK;
}

int mv_linear_mp_wgrad(const float* g, const float* x, float* dw, int64_t M, int N, int K, mv_stream_t stream) {
    MV_CHECK_ARG(g && x && dw && M > 0 && N > 0 && K > 0, "linear_mp_wgrad: bad arguments");
    MV_CHECK_ARG(N <= LMP_MAX_DIM && K <= LMP_MAX_DIM, "linear_mp_wgrad: N = %d / K = %d above %d", N, K, LMP_MAX_DIM);
    const long long out_elems = (long long)N * K;
    const long long tiles = (((long long)N + LMP_T - 1) / LMP_T) * (((long long)K + LMP_T - 1) / LMP_T);
    const LmpSplit sp = lmp_wgrad_split(tiles, M, out_elems, (hipStream_t)stream, dw);               // the M rows split over blocks
    LmpP p = {g, x, nullptr, sp.part, (long long)N, (long long)M, K, (long long)N, (long long)K, lmp_vec_ok(g, N), lmp_vec_ok(x, K), sp.chunk, 0};
    set_kernel_name(sp.split > 1 ? "linear_mp_wgrad_split_bf16" : "linear_mp_wgrad_bf16");
    const int rc = lmp_launch<true, true>(p, (int)sp.split, (hipStream_t)stream);
    if (rc != MV_OK) return rc;
    if (sp.split > 1) sum_parts((hipStream_t)stream, sp.part, dw, out_elems, (int)sp.split);
    MV_LAUNCH_CHECK();
    return MV_OK;
}

}  // extern "C"
