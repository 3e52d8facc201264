// Pieces shared by the concat-free 3x3 kernels (fire_expand.hip, inception_pair.hip, conv3x3_slice.hip) and, for the epilogue and the
// tile-row permutation, the 128 x 128 pointwise tile of pw128.h (conv1x1_split.hip, preact1x1.hip).  What a kernel keeps for itself is
// the formula it computes and its grid; the two kernels that give a workgroup ONE pair of output tiles (inception_pair.hip,
// conv3x3_slice.hip) share their k-loop too.  The few lines that string stage / offsets / k-loop / store together stay in each of
// the two: moved into one function template here (thread count as the parameter, a store functor; also with the store called
// directly, with tid and m0 passed in, with the functor by value or always_inline), conv3x3_pair_kernel took 74 VGPRs for 72 every
// time, while conv3x3_slice_kernel<2> / <4> kept their 54 and the parent's text against the same header its 72.
//
// The flat range.  m is the FLATTENED pixel index b * H * W + h * W + w of an NHWC bf16 tensor; a workgroup owns TM consecutive pixels
// from m0 on, whatever image they belong to (small maps at batch size still fill the machine).  It stages, once, slots
// m0 - W - 1 .. m0 + TM + W of S channels of the source in LDS: the tile and its one-pixel halo are all inside that range, since
// neighbour (dh, dw) of pixel m is flat pixel m + dh W + dw.  Range entries outside 0 .. M-1 are written as zeros, and one more
// all-zero slot follows the range (slot n_slots = TM + 2 W + 2): a tap that falls outside its IMAGE's map, or belongs to a pixel past
// M, reads that slot, so the padding is zeros in LDS and is never read from memory -- and no tap ever reads a neighbouring image's
// pixel.  A slot is S bf16 + 16 bytes of padding (row strides 48 / 80 / 112 / 144 .. bytes: the 16-byte reads of 16 consecutive pixels
// fall on 16 different bank quads).
//
// The product runs on v_mfma_f32_32x32x16_bf16 with the weights as the A operand (rows = output channels) and the pixels as the B
// operand (pixel = lane % 32, channels 8 (lane / 32) .. of the step); the k-step is 16 channels of ONE tap (S is a multiple of 16), so
// no step reads past a pixel's S channels.  The weights are streamed from L2 in fragment order, packed once on the host
// (ops.fire_fragments): row p of a 32-channel tile holds channel mfma32_tile_row(p), which is accumulator register
// (p % 4) + 4 (p / 8) of lane half (p / 4) % 2, so a lane ends up with 16 CONSECUTIVE output channels of its pixel in its 16
// accumulator registers: one affine step, ReLU and two 16-byte stores into the tensor's channel slice.
#pragma once
#include "mfma_common.h"

namespace mv {

// the output channel (inside its 32-channel tile) that row p of an A tile has to hold
__host__ __device__ constexpr int mfma32_tile_row(int p) { return 16 * ((p >> 2) & 1) + 4 * (p >> 3) + (p & 3); }

// LDS bytes of a TM-pixel tile on a W-wide map with S channels per pixel: the range, its halo and the zero slot
__host__ __device__ constexpr size_t flat_lds_bytes(int TM, int W, int S) { return (size_t)(TM + 2 * W + 3) * (2 * S + 16); }

// the flat range and the zero slot to LDS, NT threads: channels c0 .. c0 + 8 C8 - 1 of source rows `ld` elements apart, in 16-byte
// chunks (C8 per pixel; a compile-time constant at the call site keeps i / C8 a compile-time division)
template <int NT>
__device__ __forceinline__ void flat_stage(char* lds, const bf16_t* src, const long long ld, const int c0, const int C8, const long long m0,
                                           const int W, const long long M, const int n_slots, const int row_b, const int tid) {
    const int total = (n_slots + 1) * C8;
    const long long f0 = m0 - W - 1;
    for (int i = tid; i < total; i += NT) {
        const int slot = i / C8, c8 = i - slot * C8;
        const long long f = f0 + slot;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (slot < n_slots && f >= 0 && f < M) v = *(const uint4*)(src + f * ld + c0 + c8 * 8);
        *(uint4*)(lds + slot * row_b + c8 * 16) = v;
    }
}

// the LDS byte offsets of the nine taps of tile pixel `local` (flat pixel m0 + local) for lane half hh
__device__ __forceinline__ void flat_tap_offsets(int (&off)[9], const int local, const long long m0, const long long M, const int H,
                                                 const int W, const int n_slots, const int row_b, const int hh) {
    const long long m = m0 + local;
    const int HW = H * W;
    const bool live = m < M;
    const int rem = live ? (int)(m % HW) : 0;
    const int h = rem / W, w = rem - h * W;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int s = 0; s < 3; ++s) {
            const bool ok = live && (unsigned)(h + r - 1) < (unsigned)H && (unsigned)(w + s - 1) < (unsigned)W;
            const int slot = ok ? local + r * W + s : n_slots;
            off[r * 3 + s] = slot * row_b + hh * 16;
        }
}

// NJ 32-channel tiles x 32 pixels over the nine taps
template <int NJ>
__device__ __forceinline__ void flat_taps9(const uint4* __restrict__ wf, const char* lds, const int (&off)[9], f32x16 (&acc)[2], const int KC,
                                          const int lane) {
    // the k-steps of a tile are consecutive in the packed array whatever the tap: the fragments of step ks + 2 are requested while
    // step ks runs (the index is clamped to the last step, so nothing past the tile is read)
    const int KS = 9 * KC;
    const uint4* wl = wf + lane;
    const uint4* wh = wl + (NJ == 2 ? KS * 64 : 0);
    uint4 n0a = wl[0], n0b = wh[0], n1a = wl[64], n1b = wh[64];
    int ks = 0;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
        const char* bp = lds + off[tap];
        for (int kc = 0; kc < KC; ++kc, ++ks) {
            const bf16x8 a0 = __builtin_bit_cast(bf16x8, n0a), a1 = __builtin_bit_cast(bf16x8, n0b);
            n0a = n1a;
            n0b = n1b;
            const int nx = (ks + 2 < KS ? ks + 2 : KS - 1) * 64;
            n1a = wl[nx];
            if (NJ == 2) n1b = wh[nx];
            const bf16x8 b = __builtin_bit_cast(bf16x8, *(const uint4*)(bp + kc * 32));
            acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b, acc[0], 0, 0, 0);
            if (NJ == 2) acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b, acc[1], 0, 0, 0);
        }
    }
}

// relu(a * scale + shift), the lane holding channels 0 .. 15 from `dst` on (accumulator registers 0 .. 15 in that order); the
// bounds checks are the caller's.  fire_expand.hip keeps its own epilogue (a + bias, a null bias, its check): routed through this
// function, as a template on the arithmetic, with the check in front of the call or in a wrapper, its four 256-pixel instantiations
// took 118 VGPRs for 115 / 116; only the check and the arithmetic in ONE function gave the old figures.
__device__ __forceinline__ void store16_relu(const f32x16& a, const float* scale, const float* shift, bf16_t* dst) {
    uint32_t o[8];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const float4 s = *(const float4*)(scale + 4 * g), h = *(const float4*)(shift + 4 * g);
        o[2 * g] = pack_bf2(fmaxf(fmaf(a[4 * g], s.x, h.x), 0.f), fmaxf(fmaf(a[4 * g + 1], s.y, h.y), 0.f));
        o[2 * g + 1] = pack_bf2(fmaxf(fmaf(a[4 * g + 2], s.z, h.z), 0.f), fmaxf(fmaf(a[4 * g + 3], s.w, h.w), 0.f));
    }
    uint4* d = (uint4*)dst;
    d[0] = make_uint4(o[0], o[1], o[2], o[3]);
    d[1] = make_uint4(o[4], o[5], o[6], o[7]);
}

// the identity form: the 16 values rounded to bf16 and stored as they are (a convolution with nothing behind it: negatives survive)
__device__ __forceinline__ void store16_plain(const f32x16& a, bf16_t* dst) {
    uint32_t o[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = pack_bf2(a[2 * e], a[2 * e + 1]);
    uint4* d = (uint4*)dst;
    d[0] = make_uint4(o[0], o[1], o[2], o[3]);
    d[1] = make_uint4(o[4], o[5], o[6], o[7]);
}

}  // namespace mv
