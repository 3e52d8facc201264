// Pieces shared by the accumulator-layout boundary kernels (chain_rc.hip: chain_rc, chain_res; chain_l2.hip): the fragment and shift
// operands in LDS (host: ops.chain_acc_operands), accumulator quads <-> packed bf16, the launch tail.  What a kernel keeps for itself
// is its schedule -- which fragment a step takes, what is in flight, where the barriers are -- and everything that touches its
// wave's LDS patch: the row-major staging and stores were tried as helpers here too and did not compile to the same code (a patch
// pointer handed to a function went through a generic address: null checks against the shared aperture, ds_write2_b32 for
// ds_write_b64, up to 8 more VGPRs), so each kernel spells those out.
#pragma once
#include "mfma_common.h"

namespace mv {

// fragments -> LDS: a straight copy (the host packed them in consumption order), several loads in flight per thread; the index is
// clamped instead of branching around the load
template <int NFRAG, int NT>
__device__ __forceinline__ void acc_copy_fragments(char* dst, const bf16_t* wf, int tid) {
    constexpr int N16 = NFRAG * 64, U = 4;
    for (int base = 0; base < N16; base += U * NT) {
        uint4 v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int i = base + u * NT + tid;
            v[u] = ((const uint4*)wf)[i < N16 ? i : N16 - 1];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int i = base + u * NT + tid;
            if (i < N16) ((uint4*)dst)[i] = v[u];
        }
    }
}

// The A operands in LDS.  Fragment f of region `half` = 64 lanes x 16 bytes at f KB: one conflict-free ds_read_b128.  The two regions
// are whatever the kernel keeps there: the halves of one resident table (second = 64 KB, fragment f -> (f >> 6, f & 63)) or two chunk
// buffers (second = the chunk size).  Shift row r = 64 words at shift_rows + 256 r: word r' < 32 = [hi(shift[row r']) | lo << 16],
// words 32 .. 63 zero.
// The bases are OPAQUE 32-bit addresses, so that every read is base + compile-time immediate.  (Left to itself hipcc materialised one
// address register per table read and spilled them; scratch reloads count in vmcnt and put `s_waitcnt vmcnt(0)` between the MFMAs.)
struct AccOperands {
    typedef __attribute__((address_space(3))) const char* lds_cp;
    unsigned wb0, wb1, sbase;
    bf16x8 ones;                                                 // B of a shift step: k-slots 0 and 1 (lanes fh = 0) are 1.0

    // frags: the first region; the second one and the shift rows lie `second` and `shift_rows` bytes behind it
    __device__ __forceinline__ AccOperands(const char* frags, unsigned second, unsigned shift_rows, int lane) {
        wb0 = (unsigned)(uintptr_t)(lds_cp)frags + lane * 16;
        wb1 = wb0 + second;
        sbase = (unsigned)(uintptr_t)(lds_cp)frags + shift_rows + lane * 4;
        asm volatile("" : "+v"(wb0), "+v"(wb1), "+v"(sbase));
        u32x4_t o;
        o[0] = (lane >> 5) ? 0u : 0x3f803f80u; o[1] = 0u; o[2] = 0u; o[3] = 0u;
        ones = __builtin_bit_cast(bf16x8, o);
    }
    __device__ __forceinline__ bf16x8 afrag(int half, int f) const {
        const lds_cp b = (lds_cp)(uintptr_t)(half ? wb1 : wb0);
        return __builtin_bit_cast(bf16x8, *(const __attribute__((address_space(3))) u32x4_t*)(b + f * 1024));
    }
    // A of a shift step: lane r < 32 holds [hi(shift[row r]), lo(shift[row r]), 0 x 6], lanes 32 .. 63 zeros
    __device__ __forceinline__ bf16x8 sfrag(int row) const {
        u32x4_t v;
        v[0] = *(const __attribute__((address_space(3))) unsigned*)((lds_cp)(uintptr_t)sbase + row * 256);
        v[1] = 0u; v[2] = 0u; v[3] = 0u;
        return __builtin_bit_cast(bf16x8, v);
    }
    // acc + shift row: the shift enters through the matrix pipe as one more k-step (two bf16 terms: 16 mantissa bits)
    __device__ __forceinline__ f32x16 add_shift(int row, f32x16 acc) const {
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(sfrag(row), ones, acc, 0, 0, 0);
    }
    __device__ __forceinline__ f32x16 shift(int row) const {     // an accumulation that starts at its shift
        f32x16 z;
#pragma unroll
        for (int e = 0; e < 16; ++e) z[e] = 0.f;
        return add_shift(row, z);
    }
};

// ---- a 32-channel chunk in the accumulator layout: lane (fr, fh) holds, per quad g, channels 8 g + 4 fh .. + 3 of pixel fr; as
// bf16 that is the 8 packed words pk[2 g], pk[2 g + 1]
__device__ __forceinline__ void acc_set_quad(f32x16& a, int g, uint32_t x, uint32_t y) {      // four bf16 -> accumulator floats
    a[4 * g] = __uint_as_float(x << 16);
    a[4 * g + 1] = __uint_as_float(x & 0xffff0000u);
    a[4 * g + 2] = __uint_as_float(y << 16);
    a[4 * g + 3] = __uint_as_float(y & 0xffff0000u);
}
// pk[2 g], pk[2 g + 1] = bf16(relu(quad g of a)) (relu_pack_bf2: half a conversion + half a max per value)
__device__ __forceinline__ void acc_relu_pack_quad(const f32x16& a, int g, uint32_t* pk) {
    pk[2 * g] = relu_pack_bf2(a[4 * g], a[4 * g + 1]);
    pk[2 * g + 1] = relu_pack_bf2(a[4 * g + 2], a[4 * g + 3]);
}

// ---- host: up to one workgroup per CU, each walking its share of the 32-pixel tiles
inline int chain_acc_grid(int tiles_m, int waves) {
    const int need = (tiles_m + waves - 1) / waves;
    return need < 256 ? need : 256;
}
template <auto KERN, int WAVES, int SMEM, typename P>
static int chain_acc_go(const P& p, int gx, hipStream_t st) {
    static_assert(SMEM <= 160 * 1024, "LDS");
    static LdsAttrSite attr;                                     // one per kernel instance
    MV_HIP(attr.ensure((const void*)KERN, SMEM));
    hipLaunchKernelGGL(KERN, dim3(gx), dim3(WAVES * 64), SMEM, st, p);
    MV_LAUNCH_CHECK();
    return MV_OK;
}

}  // namespace mv
