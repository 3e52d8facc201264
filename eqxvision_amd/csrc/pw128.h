// The 128 x 128 pointwise tile shared by the concat-free 1x1 kernels (conv1x1_split.hip, preact1x1.hip).  What a kernel keeps for
// itself is what a B-operand piece is, what happens to it on its way into LDS, and where a lane's 16 output channels are stored.
//
//   v[m, n] = sum_{c<C} w[n][c] b[m][c]          m < M, n < N;  w row-major [N][C] bf16, b whatever the kernel's stager makes of x
//
// A 256-thread workgroup owns 128 rows (pixels, blockIdx.x) x 128 columns (output channels, blockIdx.y); the four waves are a 2 x 2
// grid of 64 x 64 sub-tiles on v_mfma_f32_32x32x16_bf16 with the weights as the A operand (rows = output channels) and the pixels as
// the B operand.  The lane reads weight row mfma32_tile_row(lane % 32) of its 32-row tile, so its 16 accumulator registers are 16
// CONSECUTIVE output channels of one pixel (flat3x3.h: store16_relu / store16_plain).
//
// The reduction runs in chunks of 64 channels.  Both operands of a chunk are staged in LDS, the 128 pixel rows first, the 128 weight
// rows behind them.  The row pitch is 128 + 16 bytes: the 16-byte reads of 32 consecutive rows fall on different bank quads.  The
// chunks are double buffered: the next chunk's global loads are issued in front of the current chunk's MFMAs and stay in flight in
// registers while the matrix cores work; behind the MFMAs they are written to the OTHER buffer, which is free because every wave
// left it before the previous barrier.  So there is one barrier per chunk.  Rows past M, columns past N and channels past C are zeros
// in LDS and are never read from memory; a wave whose 64 columns are all past N only stages.
#pragma once
#include "flat3x3.h"

namespace mv {

constexpr int PW_THREADS = 256;
constexpr int PW_TM = 128, PW_TN = 128, PW_KC = 64;
constexpr int PW_ROW_B = 2 * PW_KC + 16;
constexpr int PW_BUF_B = (PW_TM + PW_TN) * PW_ROW_B;
constexpr int PW_LDS = 2 * PW_BUF_B;

__device__ __forceinline__ long long pw128_m0() { return (long long)blockIdx.x * PW_TM; }      // the workgroup's first row
__device__ __forceinline__ int pw128_n0() { return blockIdx.y * PW_TN; }                       // ... and first column

// staging: the thread moves 16-byte piece `sc8` (channels k0 + 8 sc8 ..) of rows sr + 32 j, j < 4, of both operands; in a chunk's
// buffer the B operand's rows start at row 0, the A operand's at row PW_TM
struct PwStageMap {
    const int sr = threadIdx.x >> 3, sc8 = threadIdx.x & 7;
    __device__ __forceinline__ void put(char* buf, const int at, const int j, const uint4 v) const {
        *(uint4*)(buf + (at + sr + 32 * j) * PW_ROW_B + sc8 * 16) = v;
    }
};

// rows r0 .. r0 + 127 of a row-major [R][C] bf16 matrix as they are, zeros past R and past C, to operand rows `at` ..: the weight half
// of every kernel, and the B operand of a kernel that takes its pixels as they are
struct PwRowStager {
    const bf16_t* a;
    const long long R, r0;
    const int C, at;
    const PwStageMap map;
    uint4 v[4];
    __device__ __forceinline__ void fetch(const int k0) {
        const int k = k0 + map.sc8 * 8;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long long r = r0 + map.sr + 32 * j;
            v[j] = make_uint4(0, 0, 0, 0);
            if (k < C && r < R) v[j] = *(const uint4*)(a + r * C + k);
        }
    }
    __device__ __forceinline__ void stash(char* buf) const {
#pragma unroll
        for (int j = 0; j < 4; ++j) map.put(buf, at, j, v[j]);
    }
};

// acc[channel tile j][pixel tile q] = the workgroup's product.  `bs` stages the B operand: bs.fetch(k0) issues the global loads of
// channels k0 .. k0 + 63 of the workgroup's 128 rows, bs.stash(buf) writes them through PwStageMap::put(buf, 0, ..).
template <class BStager>
__device__ __forceinline__ void pw128_product(f32x16 (&acc)[2][2], char* smem, BStager& bs, const bf16_t* w, const int C, const int N) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = wave & 1, wn = wave >> 1;
    const int hh = lane >> 5, pl = lane & 31;
    PwRowStager ws{w, N, pw128_n0(), C, PW_TM};
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[j][q][e] = 0.f;

    const bool wave_live = pw128_n0() + wn * 64 < N;
    const int a_off = (PW_TM + wn * 64 + mfma32_tile_row(pl)) * PW_ROW_B + hh * 16;
    const int b_off = (wm * 64 + pl) * PW_ROW_B + hh * 16;
    const int nchunks = (C + PW_KC - 1) / PW_KC;
    ws.fetch(0);                                                    // the weights first: behind a stager that waits for loads of
    bs.fetch(0);                                                    // its own (preact1x1.hip) they were issued one at a time
    bs.stash(smem);
    ws.stash(smem);
    __syncthreads();
    for (int ch = 0; ch < nchunks; ++ch) {
        const char* cur = smem + (ch & 1) * PW_BUF_B;
        const bool more = ch + 1 < nchunks;
        if (more) {
            ws.fetch((ch + 1) * PW_KC);
            bs.fetch((ch + 1) * PW_KC);
        }
        if (wave_live) {
            const int left = (C - ch * PW_KC) >> 4;                 // C is a multiple of 16: the last chunk may hold 1 .. 3 k-steps
            const int nks = left < 4 ? left : 4;
            for (int ks = 0; ks < nks; ++ks) {
                const bf16x8 a0 = __builtin_bit_cast(bf16x8, *(const uint4*)(cur + a_off + ks * 32));
                const bf16x8 a1 = __builtin_bit_cast(bf16x8, *(const uint4*)(cur + a_off + 32 * PW_ROW_B + ks * 32));
                const bf16x8 b0 = __builtin_bit_cast(bf16x8, *(const uint4*)(cur + b_off + ks * 32));
                const bf16x8 b1 = __builtin_bit_cast(bf16x8, *(const uint4*)(cur + b_off + 32 * PW_ROW_B + ks * 32));
                acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b0, acc[0][0], 0, 0, 0);
                acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b0, acc[1][0], 0, 0, 0);
                acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b1, acc[0][1], 0, 0, 0);
                acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b1, acc[1][1], 0, 0, 0);
            }
        }
        if (more) {
            char* nxt = smem + ((ch + 1) & 1) * PW_BUF_B;
            bs.stash(nxt);
            ws.stash(nxt);
        }
        __syncthreads();
    }
}

// store(acc[j][q], m, n) for each of the lane's four 16-channel groups that exists: row m < M, first column n < N (N is a multiple
// of 16, so the whole group does)
template <class Store>
__device__ __forceinline__ void pw128_epilogue(const f32x16 (&acc)[2][2], const long long M, const int N, Store&& store) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = wave & 1, wn = wave >> 1;
    const int hh = lane >> 5, pl = lane & 31;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int n = pw128_n0() + wn * 64 + j * 32 + 16 * hh;
        if (n >= N) continue;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const long long m = pw128_m0() + wm * 64 + q * 32 + pl;
            if (m >= M) continue;
            store(acc[j][q], m, n);
        }
    }
}

}  // namespace mv
