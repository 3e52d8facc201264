// What the mixed-precision attention kernels share (attn_mp.hip, swin_attn_mp.hip): the bf16 LDS image of an fp32 operand, its two
// fragment readers for v_mfma_f32_32x32x16_bf16 and the fp32 row store.  __forceinline__ pieces only.
//
// LDS images: one [rows][dh] bf16 image per operand, row pitch 2 dh + 16 bytes (an odd number of 16-byte slots: the row-contiguous
// ds_read_b128 fragments are conflict-free), rows >= N zero.  A product whose reduction runs along dh reads both operands as
// row-contiguous fragments (amp_frag_c); a product whose reduction runs along the staged rows reads the image with
// ds_read_b64_tr_b16 (amp_frag_t), its rows listed in the order in which the other operand -- an accumulator packed by p_frag
// (swin_attn_core.h) -- holds them.  No transposed copy is staged.
#pragma once
#include "swin_attn_core.h"      // p_frag: the accumulator -> operand pack (and the register / row order, written there)

namespace mv {

constexpr float AMP_LOG2E = 1.4426950408889634f;

template <int DH> constexpr int amp_pitch() { return DH * 2 + 16; }

typedef short amp_s16x4 __attribute__((ext_vector_type(4)));
typedef short amp_s16x8 __attribute__((ext_vector_type(8)));

// rows 0 .. NP - 1 of an fp32 operand (DH floats per row, row r at `row_of(r)`: contiguous or gathered) -> its bf16 image; rows >= N
// are zero and `row_of` is not asked for them
template <int DH, typename RowOf> __device__ __forceinline__ void amp_stage(char* img, int N, int NP, RowOf row_of) {
    constexpr int CH = DH / 4;
    for (int i = threadIdx.x; i < NP * CH; i += blockDim.x) {
        const int row = i / CH, c = i - row * CH;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (row < N) v = *(const float4*)(row_of(row) + 4 * c);
        uint2 w;
        w.x = pack_bf2(v.x, v.y);
        w.y = pack_bf2(v.z, v.w);
        *(uint2*)(img + row * amp_pitch<DH>() + c * 8) = w;
    }
}

// fragment of a product that reduces along dh: lane (fr, fh) gets elements 16 kk + 8 fh .. + 7 of row `row0 + fr`
template <int DH> __device__ __forceinline__ bf16x8 amp_frag_c(const char* img, int row0, int kk, int lane) {
    return *(const bf16x8*)(img + (row0 + (lane & 31)) * amp_pitch<DH>() + kk * 32 + (lane >> 5) * 16);
}

// fragment of a product that reduces along the image's ROWS: lane (fr, fh) gets column d0 + fr of rows row0 + 4 fh + {0..3, 8..11},
// the order of registers 0 .. 7 of an accumulator half (p_frag).  Per 16-lane group, lane 4 q + p supplies the address of row q,
// columns 4 p .. 4 p + 3 of a 4 x 16 block and receives column (lane & 15) of the four rows (linear_mp_tile.h: lmp_frag).
template <int DH> __device__ __forceinline__ bf16x8 amp_frag_t(const char* img, int row0, int d0, int lane) {
    const int gl = lane & 15, q = gl >> 2, p = gl & 3;
    const int cb = d0 + 16 * ((lane >> 4) & 1) + 4 * p;
    const char* a = img + (row0 + 4 * (lane >> 5) + q) * amp_pitch<DH>() + cb * 2;
    const amp_s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) amp_s16x4*)a);
    const amp_s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) amp_s16x4*)(a + 8 * amp_pitch<DH>()));
    const amp_s16x8 f = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(bf16x8, f);
}

__device__ __forceinline__ void amp_zero(f32x16& a) {
#pragma unroll
    for (int e = 0; e < 16; ++e) a[e] = 0.f;
}

// the lane's 8 fp32 values at p, rounded: one B operand of a product that reduces along dh, straight from memory
__device__ __forceinline__ bf16x8 amp_frag_mem(const float* p) {
    const float4 a = *(const float4*)p, c = *(const float4*)(p + 4);
    uint4 f;
    f.x = pack_bf2(a.x, a.y); f.y = pack_bf2(a.z, a.w); f.z = pack_bf2(c.x, c.y); f.w = pack_bf2(c.z, c.w);
    return __builtin_bit_cast(bf16x8, f);
}

// the lane's 16 / 32 results of one token (register 4 g + i of acc[dt] = channel 32 dt + 8 g + 4 fh + i) as fp32, times `mul`
template <int DT> __device__ __forceinline__ void amp_store_row(float* row, const f32x16 (&acc)[DT], float mul, int fh) {
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int g = 0; g < 4; ++g)
            *(float4*)(row + dt * 32 + 8 * g + 4 * fh) =
                make_float4(acc[dt][4 * g] * mul, acc[dt][4 * g + 1] * mul, acc[dt][4 * g + 2] * mul, acc[dt][4 * g + 3] * mul);
}

inline bool amp_aligned(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace mv
