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
// The LDS images, the staging helpers, the fragment reads and the MFMA step are linear_mp_tile.h (shared with conv_mp.hip).
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
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
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

    float4 va[4], vb[4];
    auto gload = [&](int s) {
        const long long r0 = rbeg + (long long)s * LMP_S;
        const int left = (int)(rend - r0 < LMP_S ? rend - r0 : LMP_S);
        if (TA) lmp_gload<true>(va, abase + r0 * p.lda, p.lda, p.vec_a, rows_a, 0, left, t);
        else    lmp_gload<false>(va, abase, p.lda, p.vec_a, rows_a, (int)r0, left, t);
        if (TB) lmp_gload<true>(vb, bbase + r0 * p.ldb, p.ldb, p.vec_b, rows_b, 0, left, t);
        else    lmp_gload<false>(vb, bbase, p.ldb, p.vec_b, rows_b, (int)r0, left, t);
    };

    f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[a][b][e] = 0.f;

    const int wr = (wave >> 1) * 64, wc = (wave & 1) * 64;
    if (steps > 0) {
        gload(0);
        lmp_lstore<TA>(lds[0][0], va, t);
        lmp_lstore<TB>(lds[0][1], vb, t);
    }
    __syncthreads();
    for (int s = 0; s < steps; ++s) {
        const int cur = s & 1;
        const bool more = s + 1 < steps;
        if (more) gload(s + 1);
        lmp_mma_step<TA, TB>(acc, lds[cur][0], lds[cur][1], wr, wc, lane);
        if (more) {                          // the other buffer was last read in step s - 1, a barrier ago
            lmp_lstore<TA>(lds[cur ^ 1][0], va, t);
            lmp_lstore<TB>(lds[cur ^ 1][1], vb, t);
        }
        __syncthreads();
    }

    // C/D map of the 32x32 MFMA: column = lane & 31, row = (e & 3) + 8 (e >> 2) + 4 (lane >> 5): a register is one 128-byte row segment
    float* cpart = p.c + (long long)blockIdx.y * p.I * p.J;
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        const int j = j0 + wc + 32 * b + (lane & 31);
        const bool jok = j < p.J;
        const float bj = (p.bias && jok) ? p.bias[j] : 0.f;
#pragma unroll
        for (int a = 0; a < 2; ++a) {
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const long long i = i0 + wr + 32 * a + (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
                if (jok && i < p.I) cpart[i * p.J + j] = acc[a][b][e] + bj;
            }
        }
    }
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
    // rows split over blocks: ~4 workgroups per CU, every part at least 256 rows (8 steps), at most 64 parts
    const long long steps = ((long long)M + LMP_S - 1) / LMP_S;
    long long split = tiles >= 1024 ? 1 : (1024 + tiles - 1) / tiles;
    if (split > steps / 8) split = steps / 8;
    if (split > 64) split = 64;
    float* part = dw;
    if (split > 1) {
        // the parts live BEHIND the first 4096 bytes of the offer (the arrival words of the forward's split-K protocol, which stay zero)
        size_t have = 0;
        void* sc = peek_scratch((hipStream_t)stream, &have);
        have = have > SCRATCH_SYNC_BYTES ? have - SCRATCH_SYNC_BYTES : 0;
        const long long fit = sc ? (long long)(have / ((size_t)out_elems * 4)) : 0;
        if (fit < 2) split = 1;
        else {
            if (split > fit) split = fit;
            part = (float*)((char*)take_scratch((hipStream_t)stream, SCRATCH_SYNC_BYTES + (size_t)split * out_elems * 4) + SCRATCH_SYNC_BYTES);
        }
    }
    if (split < 1) split = 1;
    long long chunk = ((steps + split - 1) / split) * LMP_S;
    split = ((long long)M + chunk - 1) / chunk;                  // no empty part
    if (split <= 1) part = dw;
    LmpP p = {g, x, nullptr, part, (long long)N, (long long)M, K, (long long)N, (long long)K, lmp_vec_ok(g, N), lmp_vec_ok(x, K), chunk, 0};
    set_kernel_name(split > 1 ? "linear_mp_wgrad_split_bf16" : "linear_mp_wgrad_bf16");
    const int rc = lmp_launch<true, true>(p, (int)split, (hipStream_t)stream);
    if (rc != MV_OK) return rc;
    if (split > 1)
        hipLaunchKernelGGL(lmp_sum_parts_kernel, dim3((unsigned)((out_elems + 255) / 256)), dim3(256), 0, (hipStream_t)stream, part, dw,
                           out_elems, (int)split);
    MV_LAUNCH_CHECK();
    return MV_OK;
}

}  // extern "C"
