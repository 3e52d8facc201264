// The 128 x 128 x 32 bf16 tile of the mixed-precision training kernels (linear_mp.hip, conv_mp.hip): staging of an fp32 operand patch
// through registers into its bf16 LDS image, the MFMA fragments read back from it, one k-step of 32 on v_mfma_f32_32x32x16_bf16, the
// double-buffered loop over a tile's reduction (lmp_reduce), the store of a tile (lmp_store_tile) and, on the host, how a weight
// gradient splits its reduction over parts (lmp_wgrad_split).  A kernel keeps what is its own: which tile a block computes, its range of
// the reduction, how its two patches are loaded and where its output lies.
//
// LDS images (bf16), both 10240 bytes per operand and buffer:
//   contiguous operand  [128 rows][32 k] with 80-byte rows: a lane's fragment is one ds_read_b128 at row * 80 + 32 * ks + 16 * h; the
//                       rows of 16 consecutive lanes start 20 dwords apart, i.e. on 16 distinct 4-dword bank groups
//   row-axis operand    [32 k][128 columns] with 320-byte rows (256 + 64 pad): 320 B = 80 dwords = 16 (mod 64), so the 4 rows x 2
//                       sixteen-column blocks a 32-lane half reads in one ds_read_b64_tr_b16 fall on 4 x 16 = 64 distinct banks.
//                       (The padding does for plain rows what the XOR swizzle does for un-padded 256-byte rows.)
#pragma once
#include "mfma_common.h"

namespace mv {
namespace {

constexpr int LMP_T = 128;            // tile edge (outputs)
constexpr int LMP_S = 32;             // reduction elements per step
constexpr int LMP_ROW_C = 80;         // bytes per row of a contiguous operand's image  [128][32 bf16 + pad]
constexpr int LMP_ROW_T = 320;        // bytes per row of a row-axis operand's image    [32][128 bf16 + pad]
constexpr int LMP_IMG = 10240;        // bytes per operand image (128 * 80 == 32 * 320)

__device__ __forceinline__ float buf_load_f1(brsrc_t r, unsigned vo) {
    return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(r, vo, 0, 0));
}

typedef short s16x4_t __attribute__((ext_vector_type(4)));
typedef short s16x8_t __attribute__((ext_vector_type(8)));

// The operand's next [128 x 32] fp32 patch in registers: 4 chunks of 4 consecutive floats per thread.
//   contiguous: chunk c = t + 256 u -> row c >> 3 (0..127), reduction elements 4 (c & 7) .. + 3
//   row-axis:   chunk c = t + 256 u -> reduction row c >> 5 (0..31), columns 4 (c & 31) .. + 3
// `base` points at the tile's first row (contiguous: element [i0][0]; row-axis: element [r0][i0], advanced by the caller per step).
template <bool TR>
__device__ __forceinline__ void lmp_gload(float4 (&v)[4], const float* base, long long ld, bool vec, int rows_left, int red0, int red_left,
                                          int t) {
    // rows_left: valid tile rows / columns from the tile's origin on (may exceed 128); red_left: valid reduction elements from red0 on
    const brsrc_t rs = make_brsrc(base);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int c = t + 256 * u;
        int row, col, row_ok_n, col_ok_n;               // row: index along the pitch; col: first of 4 contiguous elements
        if (TR) { row = c >> 5; col = 4 * (c & 31); row_ok_n = red_left; col_ok_n = rows_left; }
        else    { row = c >> 3; col = red0 + 4 * (c & 7); row_ok_n = rows_left; col_ok_n = red0 + red_left; }
        const unsigned off = (unsigned)(((long long)row * ld + col) * 4);
        const bool rok = row < row_ok_n;
        if (vec) {
            v[u] = buf_load_f4(rs, (rok && col < col_ok_n) ? off : BUF_OOB);       // pitch % 4 == 0: a chunk is all in or all out
        } else {
            v[u].x = buf_load_f1(rs, (rok && col + 0 < col_ok_n) ? off : BUF_OOB);
            v[u].y = buf_load_f1(rs, (rok && col + 1 < col_ok_n) ? off + 4 : BUF_OOB);
            v[u].z = buf_load_f1(rs, (rok && col + 2 < col_ok_n) ? off + 8 : BUF_OOB);
            v[u].w = buf_load_f1(rs, (rok && col + 3 < col_ok_n) ? off + 12 : BUF_OOB);
        }
    }
}

// round to bf16 (RNE) and store the patch into the operand's LDS image
template <bool TR> __device__ __forceinline__ void lmp_lstore(char* img, const float4 (&v)[4], int t) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int c = t + 256 * u;
        const int off = TR ? (c >> 5) * LMP_ROW_T + (c & 31) * 8 : (c >> 3) * LMP_ROW_C + (c & 7) * 8;
        uint2 w;
        w.x = pack_bf2(v[u].x, v[u].y);
        w.y = pack_bf2(v[u].z, v[u].w);
        *(uint2*)(img + off) = w;
    }
}

// The 32x32x16 operand fragment of tile rows row0 .. row0 + 31 for k-step ks (0 / 1) of the image: lane l (r = l & 31, h = l >> 5) gets
// element j = reduction index 16 ks + 8 h + j of row row0 + r.
template <bool TR> __device__ __forceinline__ bf16x8 lmp_frag(const char* img, int row0, int ks, int lane) {
    const int h = lane >> 5;
    if (!TR) {
        return *(const bf16x8*)(img + (row0 + (lane & 31)) * LMP_ROW_C + 32 * ks + 16 * h);
    } else {
        // per 16-lane group: lane 4 q + p supplies the address of reduction row q, columns 4 p .. 4 p + 3 of a 4 x 16 block; lane i of
        // the group receives column i of the 4 rows.  Lanes 16 .. 31 / 48 .. 63 take the second 16 columns.
        const int gl = lane & 15, q = gl >> 2, p = gl & 3;
        const int cb = row0 + 16 * ((lane >> 4) & 1) + 4 * p;
        const char* a = img + (16 * ks + 8 * h + q) * LMP_ROW_T + cb * 2;
        const s16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)a);
        const s16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)(a + 4 * LMP_ROW_T));
        const s16x8_t f = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        return __builtin_bit_cast(bf16x8, f);
    }
}

// One step of 32 reduction elements on a wave's 64 x 64 outputs (rows wr .., columns wc .. of the tile): 2 x 2 MFMA tiles, 2 k-steps of 16.
template <bool TA, bool TB>
__device__ __forceinline__ void lmp_mma_step(f32x16 (&acc)[2][2], const char* img_a, const char* img_b, int wr, int wc, int lane) {
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
        const bf16x8 a0 = lmp_frag<TA>(img_a, wr, ks, lane), a1 = lmp_frag<TA>(img_a, wr + 32, ks, lane);
        const bf16x8 b0 = lmp_frag<TB>(img_b, wc, ks, lane), b1 = lmp_frag<TB>(img_b, wc + 32, ks, lane);
        acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b0, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b1, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b0, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b1, acc[1][1], 0, 0, 0);
    }
}

// The reduction of one 128 x 128 tile over `steps` steps of 32: LDS double-buffered with the next step's patches in flight in registers,
// one barrier per step.  load(va, vb) fills the two patches of the next step: it is called exactly once per step, in step order, and keeps
// its own place in the reduction between calls.  Clears acc; wave w of the 4 owns rows 64 (w >> 1) .., columns 64 (w & 1) .. .
template <bool TA, bool TB, class Load>
__device__ __forceinline__ void lmp_reduce(f32x16 (&acc)[2][2], char (&lds)[2][2][LMP_IMG], int steps, int t, Load&& load) {
    const int lane = t & 63, wave = t >> 6;
    const int wr = (wave >> 1) * 64, wc = (wave & 1) * 64;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[a][b][e] = 0.f;

    float4 va[4], vb[4];
    if (steps > 0) {
        load(va, vb);
        lmp_lstore<TA>(lds[0][0], va, t);
        lmp_lstore<TB>(lds[0][1], vb, t);
    }
    __syncthreads();
    for (int s = 0; s < steps; ++s) {
        const int cur = s & 1;
        const bool more = s + 1 < steps;
        if (more) load(va, vb);
        lmp_mma_step<TA, TB>(acc, lds[cur][0], lds[cur][1], wr, wc, lane);
        if (more) {                          // the other buffer was last read in step s - 1, a barrier ago
            lmp_lstore<TA>(lds[cur ^ 1][0], va, t);
            lmp_lstore<TB>(lds[cur ^ 1][1], vb, t);
        }
        __syncthreads();
    }
}

// Stores a tile (+ bias[j], fp32, if given).  C/D map of the 32x32 MFMA: column = lane & 31, row = (e & 3) + 8 (e >> 2) + 4 (lane >> 5): a
// register is one 128-byte row segment.  `ctile` points at column 0 of the tile's first row, `rows` (<= 128) of which exist; the columns
// are j0 .. below J.  Offsets from ctile are 32-bit: 128 rows of a pitch of at most LMP_MAX_DIM stay below 2^28 elements, whatever the
// number of rows of the whole output.
__device__ __forceinline__ void lmp_store_tile(const f32x16 (&acc)[2][2], float* ctile, unsigned ldc, int rows, int j0, int J,
                                               const float* bias, int t) {
    const int lane = t & 63, wave = t >> 6;
    const int wc = (wave & 1) * 64, row = (wave >> 1) * 64 + 4 * (lane >> 5);          // this lane's first row
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        const int j = j0 + wc + 32 * b + (lane & 31);
        const bool jok = j < J;
        const float bj = (bias && jok) ? bias[j] : 0.f;
        const unsigned off = (unsigned)row * ldc + (unsigned)j;
#pragma unroll
        for (int a = 0; a < 2; ++a) {
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int up = 32 * a + (e & 3) + 8 * (e >> 2);                        // the same for every lane: a scalar base
                if (jok && row + up < rows) (ctile + (size_t)up * ldc)[off] = acc[a][b][e] + bj;
            }
        }
    }
}

inline int lmp_vec_ok(const float* ptr, long long pitch) { return ((uintptr_t)ptr & 15) == 0 && (pitch & 3) == 0; }

// the largest pitch of a contiguous operand whose 128-row tile stays below 2^31 bytes from its descriptor's base
constexpr int LMP_MAX_DIM = 1 << 21;

// How a weight gradient of `tiles` output tiles splits its reduction of `red` elements: about 1024 workgroups (~4 per CU), every part at
// least 8 steps, at most 64 parts, no more than the scratch on offer holds (none below two: take_scratch_parts), then no empty part.
// `part`: where the kernel writes -- the parts [split][out_elems] in the scratch, or `direct` when it does not split.
struct LmpSplit {
    float* part;
    long long split, chunk;                  // parts; reduction elements per part (a multiple of LMP_S)
};
inline LmpSplit lmp_wgrad_split(long long tiles, long long red, long long out_elems, hipStream_t stream, float* direct) {
    const long long steps = (red + LMP_S - 1) / LMP_S;
    long long split = tiles >= 1024 ? 1 : (1024 + tiles - 1) / tiles;
    if (split > steps / 8) split = steps / 8;
    if (split > 64) split = 64;
    float* part = nullptr;
    if (split > 1) split = take_scratch_parts(stream, split, 2, out_elems, &part);
    if (split < 1) split = 1;
    const long long chunk = ((steps + split - 1) / split) * LMP_S;
    split = (red + chunk - 1) / chunk;
    return {split > 1 ? part : direct, split, chunk};
}

}  // namespace
}  // namespace mv
