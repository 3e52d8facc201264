// The softmax / P.V core the matrix-core window-attention kernels share (swin_attn.hip, both kernels of swin_block_attn.hip; attn.hip
// takes p_frag): __forceinline__ pieces only -- loads, tiles and pipelining stay with the kernels.
//
// Conventions, for every user.  A wave works on 32 queries x 64 keys of one (window, head); lane = (fr, fh) = (lane & 31, lane >> 5).
//   * S^T = K . Q^T (v_mfma_f32_32x32x16_bf16, A = K rows, B = Q rows) leaves ONE query per lane: query fr of the wave's query block.
//     Its 64 keys sit in two accumulators s[kt] of 16 registers, on the lane and its partner lane ^ 32:
//         register e of s[kt]  =  key 32 kt + (e & 3) + 8 (e >> 2) + 4 fh
//     i.e. register quad gq = e >> 2 holds the four consecutive keys 32 kt + 8 gq + 4 fh .. + 3: bias and region ids arrive as one
//     16-byte load per quad, and a row reduction is 32 registers + one lane ^ 32 exchange.
//   * O^T = V^T . P^T: the MFMA's reduction index only has to agree between its two operands, so step (kt, half) takes the keys of
//     registers 8 half .. 8 half + 7 of s[kt] in REGISTER order -- P feeds the B operand from the registers it sits in (p_frag), and
//     the V^T fragment of a lane lists the same keys: 32 kt + 16 half + 4 fh + {0..3, 8..11}.  Stored in "slot" order (vt_slot) these
//     are 16 contiguous bytes; stored in key order they are two 8-byte pieces 16 bytes apart.
//   * The output accumulator holds channel 8 gq + 4 fh + i of the lane's query in register 4 gq + i (store_quads_bf16).
#pragma once
#include "mfma_common.h"

namespace mv {

// registers 8 half .. 8 half + 7 of an accumulator, rounded to bf16: the B operand of one P . V step (and any other 8-register pack)
__device__ __forceinline__ bf16x8 p_frag(const f32x16& s, int half) {
    uint4 f;
    f.x = pack_bf2(s[8 * half + 0], s[8 * half + 1]);
    f.y = pack_bf2(s[8 * half + 2], s[8 * half + 3]);
    f.z = pack_bf2(s[8 * half + 4], s[8 * half + 5]);
    f.w = pack_bf2(s[8 * half + 6], s[8 * half + 7]);
    return __builtin_bit_cast(bf16x8, f);
}

// One logit, the rule every window-attention kernel shares: s * scale + relative-position bias, -100 like the reference where the
// key's mask region is not the query's, and -inf on a padded key of the tile -- padding is EXCLUDED, not masked.
__device__ __forceinline__ float win_logit(float s, float scale, float bias, bool masked, bool padded) {
    float v = fmaf(s, scale, bias);
    if (masked) v += -100.0f;
    if (padded) v = -INFINITY;
    return v;
}

// Scores -> unnormalised probabilities, in place; returns 1 / their sum.  s * scale + relative-position bias (bias_row: the query's
// 64 fp32 entries) + shift mask (-100 like the reference where key_regions[key] != qreg), exp(. - row max).
// GUARD (swin_attn.hip: any window of <= 64 tokens, bias padded with zeros): region ids are read only if `shifted`, keys >= n get
// -inf.  Without it (the block kernels) the caller's bias carries -1e30 on padded keys and its region table holds 0 when unshifted.
// one_quad: debug ablation of swin_win96 -- every quad reads the row's first 32 bytes.
template <bool GUARD>
__device__ __forceinline__ float win_softmax(f32x16 (&s)[2], float scale, const float* bias_row, const int* key_regions, int qreg, int fh,
                                             bool shifted = true, int n = 64, bool one_quad = false) {
    const bool mask = !GUARD || shifted;
    float mx = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
        for (int gq = 0; gq < 4; ++gq) {
            const int key0 = 32 * kt + 8 * gq + 4 * fh;
            const float4 bv = *(const float4*)(bias_row + (one_quad ? 4 * fh : key0));
            int4 kr = make_int4(0, 0, 0, 0);
            if (mask) kr = *(const int4*)(key_regions + key0);
            const float bb[4] = {bv.x, bv.y, bv.z, bv.w};
            const int rr[4] = {kr.x, kr.y, kr.z, kr.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float v = win_logit(s[kt][4 * gq + e], scale, bb[e], mask && rr[e] != qreg, GUARD && key0 + e >= n);
                s[kt][4 * gq + e] = v;
                mx = fmaxf(mx, v);
            }
        }
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    float sum = 0.f;
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const float pe = __expf(s[kt][e] - mx);
            s[kt][e] = pe;
            sum += pe;
        }
    sum += __shfl_xor(sum, 32);
    return 1.f / sum;
}

// O^T[d][query] = sum over the 64 keys of V^T[d][key] P[key][query]; vfrag(step) reads the lane's V^T fragment of step 2 kt + half
template <typename VFrag>
__device__ __forceinline__ f32x16 win_pv(const f32x16 (&s)[2], VFrag vfrag) {
    f32x16 o;
#pragma unroll
    for (int e = 0; e < 16; ++e) o[e] = 0.f;
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
        for (int half = 0; half < 2; ++half)
            o = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vfrag(2 * kt + half), p_frag(s[kt], half), o, 0, 0, 0);
    return o;
}

// position of token 32 tb + fr in a v^T row kept in slot order: the 8 keys a lane feeds to one P . V step sit next to each other
// (token block, pair of register quads, lane half, quad parity, key of the quad) -- lane (fr, fh) reads step st at slot 16 st + 8 fh
__device__ __forceinline__ int vt_slot(int tb, int fr) {
    const int kg = fr >> 3, khh = (fr >> 2) & 1, kr = fr & 3;
    return ((tb * 2 + (kg >> 1)) * 2 + khh) * 8 + (kg & 1) * 4 + kr;
}

// the lane's 16 channels of one token as bf16: quad gq (channels 8 gq + 4 fh .. + 3) -> 8 bytes at dst + 16 gq; dst = channel 4 fh
__device__ __forceinline__ void store_quads_bf16(char* dst, const f32x16& v) {
#pragma unroll
    for (int gq = 0; gq < 4; ++gq) {
        uint2 u;
        u.x = pack_bf2(v[4 * gq + 0], v[4 * gq + 1]);
        u.y = pack_bf2(v[4 * gq + 2], v[4 * gq + 3]);
        *(uint2*)(dst + 16 * gq) = u;
    }
}

}  // namespace mv
