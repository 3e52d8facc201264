// ResNet-50 / 101 / 152 layer 2: the block boundaries in chain_rc.hip's accumulator-layout style, for a stage whose weights do NOT
// fit in LDS (C = 128, K = 512; reference resnet.py:144-162, 295-303, 330-333).  One kernel template, three instances:
//
//   entry  (C2 = 256, RES = false): y0 = relu( [s3 W3 | sd Wd] . [t2_0 | x] + shift )           -> HBM (block 1's identity)
//                                   t1 = relu( (sN W1n) . bf16(y0) + shiftN ),  N2 = 128        -> HBM
//   middle (C2 = 0,   RES = true):  y  = relu( (s3 W3) . t2 + shift3 + res ),  t1 as above     (= chain_stream.hip's function)
//   exit   (C2 = 0,   RES = true):  the same with N2 = 256 (layer 3's conv1), y written whole or (SUB) only at even (h, w)
//
// From chain_rc.hip: weights in MFMA FRAGMENT ORDER (host: ops.chain_acc_operands), every BatchNorm scale folded into the bf16 rows, every
// shift one more k-step through the matrix pipe, the identity the C operand that STARTS y's accumulation, y kept in the accumulator
// layout so that its packed bf16 chunk IS the B operand of the next conv1 (host-side permutation of that layer's reduction index),
// the A fragments fetched RD matrix instructions ahead into a register ring, bf16 LDS patches only for the row-major stores.
// From chain_stream.hip: the weights (entry 512 KB, middle 256 KB, exit 384 KB) are STREAMED through LDS as 32-channel chunks of y --
// chunk c = the C/16 fragments of W3's rows 32 c .. 32 c + 31 followed by the 2 N2/32 fragments of W1n's columns 32 c .. (one
// contiguous FPC KB piece: the copy is linear).  All waves of a workgroup walk the chunks together, each on its own 32-pixel tile
// whose x fragments stay in registers for the whole walk; two chunk buffers in LDS, chunk c + AHEAD fetched into registers at the
// top of chunk c and written to LDS after its matrix work, ONE workgroup barrier per chunk.  The identity rows of chunk c + 1 are
// fetched at the top of chunk c (the next tile's first chunk at the last one).
// Every s_waitcnt vmcnt inside a tile must be exact: no conditional load inside a chunk step (rows are clamped, stores past the end
// get BUF_OOB), the chunk loop is unrolled by two (buffer parity is a compile-time constant), the last pair is peeled.
#include <type_traits>
#include "chain_acc.h"
#include "conv_launchers.h"

namespace mv {

struct ChainL2P {
    const bf16_t* xa;      // [M][C1] conv2 output of this block
    const bf16_t* xb;      // C2 > 0: [M][C2] the stage input, already sub-sampled to this stage's map (the downsample branch)
    const bf16_t* res;     // RES: [M][512] the identity
    const bf16_t* wf;      // 16 chunks x FPC fragments of 1 KB
    const unsigned* sh;    // 16 rows of shift3 (per chunk) + N2 / 32 rows of shiftN, as chain_rc.hip's
    bf16_t* y;             // [M][512], or SUB: [N][H/2][W/2][512]
    bf16_t* t1;            // [M][N2]
    int M, tiles_m, subH, subW, rounds, act;
};

template <int C1, int C2, bool RES, int N2, bool SUB, int WAVES, int AHEAD, int RD>
__global__ __launch_bounds__(WAVES * 64) void chain_l2_kernel(const ChainL2P p) {
    constexpr int K = 512, NCH = K / 32, KA = C1 / 16, KX = (C1 + C2) / 16, T2 = N2 / 32, FPC = KX + 2 * T2, CB = FPC * 1024,
                  NSH = NCH + T2, NT = WAVES * 64, PT = FPC * 64 / NT, PITCH = 144;
    static_assert((FPC * 64) % NT == 0 && RD <= FPC && (AHEAD == 1 || AHEAD == 2) && NCH % 2 == 0, "chain_l2 shape");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* wbuf = smem;                                           // [2][CB] chunk buffers
    unsigned* shl = (unsigned*)(smem + 2 * CB);                  // NSH shift rows of 64 words
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    char* ep = smem + 2 * CB + NSH * 256 + wave * (32 * PITCH);  // the wave's patch: 32 rows x 128 bytes

    auto wload = [&](int c, u32x4_t* wr) {                       // my 16-byte pieces of chunk c: tid, tid + NT, ...
        const u32x4_t* src = (const u32x4_t*)p.wf + c * (CB / 16);
#pragma unroll
        for (int u = 0; u < PT; ++u) wr[u] = src[u * NT + tid];
    };
    auto wstore = [&](int buf, const u32x4_t* wr) {
#pragma unroll
        for (int u = 0; u < PT; ++u) ((u32x4_t*)(wbuf + buf * CB))[u * NT + tid] = wr[u];
    };
    auto block_sync = [&]() {
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);                       // nothing of the next chunk is hoisted above the barrier
    };

    u32x4_t wreg[AHEAD][PT];                                     // chunk k travels in wreg[k % AHEAD]
    wload(0, wreg[0]);
    if constexpr (AHEAD == 2) wload(1, wreg[1]);
    for (int i = tid; i < NSH * 64; i += NT) shl[i] = p.sh[i];
    wstore(0, wreg[0]);
    block_sync();

    const int fr = lane & 31, fh = lane >> 5;
    const AccOperands lds(wbuf, CB, 2 * CB, lane);               // the two chunk buffers, then the shift rows

    auto load_x = [&](uint4* xf, int tile) {                     // xf[kk]: k-step kk of [xa | xb] for pixel fr
        int m = tile * 32 + fr;
        m = m < p.M ? m : p.M - 1;                               // clamp: rows past the end are never stored
#pragma unroll
        for (int kk = 0; kk < KA; ++kk) xf[kk] = *(const uint4*)(p.xa + (long long)m * C1 + fh * 8 + kk * 16);
#pragma unroll
        for (int kk = 0; kk < KX - KA; ++kk) xf[KA + kk] = *(const uint4*)(p.xb + (long long)m * C2 + fh * 8 + kk * 16);
    };
    struct Rows2 { uint4 r0, r1; };                              // identity rows of a chunk: row pass * 16 + lane / 4, 16 bytes per lane
    auto load_res = [&](int tile, int c) -> Rows2 {
        Rows2 o;
        if constexpr (RES) {
            auto row = [&](int pass) -> uint4 {
                int m = tile * 32 + pass * 16 + (lane >> 2);
                m = m < p.M ? m : p.M - 1;
                return *(const uint4*)(p.res + (long long)m * K + c * 32 + (lane & 3) * 8);
            };
            o.r0 = row(0); o.r1 = row(1);
        } else {
            o.r0 = make_uint4(0, 0, 0, 0); o.r1 = o.r0;
        }
        return o;
    };

    uint4 xf[KX];
    const int tbase = p.tiles_m / (int)gridDim.x, trem = p.tiles_m % (int)gridDim.x;   // block b: tiles [tile0, tile0 + nb)
    const int nb = tbase + ((int)blockIdx.x < trem ? 1 : 0);
    const int tile0 = (int)blockIdx.x * tbase + ((int)blockIdx.x < trem ? (int)blockIdx.x : trem);
    const int wv = __builtin_amdgcn_readfirstlane(wave);
    int tile = tile0 + wave;
    load_x(xf, tile);
    Rows2 rr = load_res(tile, 0);

    for (int r = 0; r < p.rounds; ++r, tile += p.act) {
        if (!(wv < p.act && r * p.act + wv < nb)) {             // no tile for this wave in this round: keep the weights moving
#pragma unroll 1
            for (int c0 = 0; c0 < NCH; c0 += 2)
#pragma unroll
                for (int ci = 0; ci < 2; ++ci) {
                    const int c = c0 + ci, cn = c + AHEAD < NCH ? c + AHEAD : c + AHEAD - NCH;
                    wload(cn, wreg[ci % AHEAD]);
                    wstore(ci ^ 1, wreg[(ci + 1) % AHEAD]);
                    block_sync();
                }
            continue;
        }
        const int tile_u = __builtin_amdgcn_readfirstlane(tile);
        const int ntile = tile + p.act;
        const brsrc_t ry = SUB ? make_brsrc(p.y) : make_brsrc(p.y + (long long)tile_u * 32 * K);
        const brsrc_t rt = make_brsrc(p.t1 + (long long)tile_u * 32 * N2);
        const int rows_left = p.M - tile_u * 32;
        unsigned yoff[2];                                        // byte offset of row pass * 16 + lane / 4 of the tile in y, or BUF_OOB
#pragma unroll
        for (int pass = 0; pass < 2; ++pass) {
            const int row = pass * 16 + (lane >> 2);
            if constexpr (SUB) {
                const int m = tile_u * 32 + row, hw = p.subH * p.subW;
                const int b = m / hw, rem = m - b * hw;
                const int h = rem / p.subW, w = rem - h * p.subW;
                yoff[pass] = m < p.M && !((h | w) & 1) ? (unsigned)(((b * (p.subH >> 1) + (h >> 1)) * (p.subW >> 1) + (w >> 1)) * K) * 2u
                                                       : BUF_OOB;
            } else {
                yoff[pass] = row < rows_left ? (unsigned)(row * K) * 2u : BUF_OOB;
            }
        }
        f32x16 acc2[T2];                                         // the next conv1's accumulators start at its shift
#pragma unroll
        for (int a2 = 0; a2 < T2; ++a2) acc2[a2] = lds.shift(NCH + a2);

        // one chunk: c & 1 == CI; LAST: the tile's last chunk, which also fetches the next round's x fragments (peeled: no branch)
        auto step = [&](auto CI, const int c, auto LAST) {
            constexpr int ci = decltype(CI)::value;
            {
                const int cn = c + AHEAD < NCH ? c + AHEAD : c + AHEAD - NCH;
                wload(cn, wreg[ci % AHEAD]);
            }
            bf16x8 ring[RD];
#pragma unroll
            for (int d = 0; d < RD; ++d) ring[d] = lds.afrag(ci, d);
            auto take = [&](int i) -> bf16x8 {                   // fragment i of the chunk; its slot is refilled with i + RD
                __builtin_amdgcn_sched_barrier(0);
                const bf16x8 a = ring[i % RD];
                if (i + RD < FPC) ring[i % RD] = lds.afrag(ci, i + RD);
                return a;
            };
            f32x16 a;
            if constexpr (RES) {                                 // identity rows -> patch -> accumulator layout; chunk c + 1's requested
                {
                    char* w = ep + (lane >> 2) * PITCH + (lane & 3) * 16;
                    *(uint4*)(w) = rr.r0; *(uint4*)(w + 16 * PITCH) = rr.r1;
                }
                wave_lds_fence();
                rr = load_res(c + 1 < NCH ? tile : ntile, c + 1 < NCH ? c + 1 : 0);   // (rows clamped: harmless behind the last tile)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const uint2 u = *(const uint2*)(ep + fr * PITCH + (8 * g + 4 * fh) * 2);
                    acc_set_quad(a, g, u.x, u.y);
                }
                wave_lds_fence();                                // the patch is free again (y staging below)
            } else {
#pragma unroll
                for (int e = 0; e < 16; ++e) a[e] = 0.f;
            }
            a = lds.add_shift(c, a);
#pragma unroll
            for (int kk = 0; kk < KX; ++kk) {
                const bf16x8 af = take(kk);
                a = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, __builtin_bit_cast(bf16x8, xf[kk]), a, 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
            uint32_t pk[8];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                pk[2 * g] = relu_pack_bf2(a[4 * g], a[4 * g + 1]);
                pk[2 * g + 1] = relu_pack_bf2(a[4 * g + 2], a[4 * g + 3]);
                *(uint2*)(ep + fr * PITCH + (8 * g + 4 * fh) * 2) = make_uint2(pk[2 * g], pk[2 * g + 1]);
            }
            if constexpr (decltype(LAST)::value) load_x(xf, ntile);
            // the next block's conv1 on this chunk: packed entries 4 s .. 4 s + 3 ARE the B operand of k-step s
#pragma unroll
            for (int q = 0; q < 2 * T2; ++q) {
                const bf16x8 af = take(KX + q);
                const int s = q / T2, a2 = q % T2;
                const uint4 b = make_uint4(pk[4 * s], pk[4 * s + 1], pk[4 * s + 2], pk[4 * s + 3]);
                acc2[a2] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, __builtin_bit_cast(bf16x8, b), acc2[a2], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
            wave_lds_fence();
#pragma unroll
            for (int pass = 0; pass < 2; ++pass) {
                const int row = pass * 16 + (lane >> 2);
                const uint4 u = *(const uint4*)(ep + row * PITCH + (lane & 3) * 16);
                buf_store_u4(ry, yoff[pass] == BUF_OOB ? BUF_OOB : yoff[pass] + (unsigned)(c * 32 + (lane & 3) * 8) * 2u, u);
            }
            wave_lds_fence();
            wstore(ci ^ 1, wreg[(ci + 1) % AHEAD]);              // chunk c + 1; that buffer was last read before the previous barrier
            block_sync();
        };
#pragma unroll 1
        for (int c0 = 0; c0 < NCH - 2; c0 += 2) {
            step(std::integral_constant<int, 0>(), c0, std::false_type());
            step(std::integral_constant<int, 1>(), c0 + 1, std::false_type());
        }
        step(std::integral_constant<int, 0>(), NCH - 2, std::false_type());
        step(std::integral_constant<int, 1>(), NCH - 1, std::true_type());

        // ---- conv1 of the next block: 32 pixels x N2 channels, 64 channels per round through the patch
#pragma unroll
        for (int rd = 0; rd < T2 / 2; ++rd) {
#pragma unroll
            for (int a2 = 0; a2 < 2; ++a2)
#pragma unroll
                for (int g = 0; g < 4; ++g)
                    *(uint2*)(ep + fr * PITCH + (a2 * 32 + 8 * g + 4 * fh) * 2) =
                        make_uint2(relu_pack_bf2(acc2[2 * rd + a2][4 * g], acc2[2 * rd + a2][4 * g + 1]),
                                   relu_pack_bf2(acc2[2 * rd + a2][4 * g + 2], acc2[2 * rd + a2][4 * g + 3]));
            wave_lds_fence();
#pragma unroll
            for (int pass = 0; pass < 4; ++pass) {
                const int row = pass * 8 + (lane >> 3);
                const uint4 u = *(const uint4*)(ep + row * PITCH + (lane & 7) * 16);
                buf_store_u4(rt, row < rows_left ? (unsigned)(row * N2 + rd * 64 + (lane & 7) * 8) * 2u : BUF_OOB, u);
            }
            wave_lds_fence();
        }
    }
}

template <int C1, int C2, bool RES, int N2, bool SUB, int WAVES, int AHEAD, int RD>
static int chain_l2_go(ChainL2P& p, long long M, hipStream_t st) {
    constexpr int FPC = (C1 + C2) / 16 + N2 / 16;
    constexpr int SMEM = 2 * FPC * 1024 + (16 + N2 / 32) * 256 + WAVES * 32 * 144;
    p.M = (int)M;
    p.tiles_m = (int)((M + 31) / 32);
    const int gx = chain_acc_grid(p.tiles_m, WAVES);
    const int per_block = (p.tiles_m + gx - 1) / gx;            // the largest share of a block
    p.rounds = (per_block + WAVES - 1) / WAVES;
    p.act = (per_block + p.rounds - 1) / p.rounds;
    return chain_acc_go<chain_l2_kernel<C1, C2, RES, N2, SUB, WAVES, AHEAD, RD>, WAVES, SMEM>(p, gx, st);
}

static bool chain_l2_m_ok(long long M) { return M >= 16384 && M < (1LL << 31) - (1 << 20); }

// middle (N2 = 128) and exit (N2 = 256) boundaries of a C = 128 / K = 512 stage: the chain_res shapes of this file
int chain_l2_res_supported(long long N, int H, int W, int C, int K, int N2, int sub, int dtype) {
    const long long M = N * H * W;
    if (!(dtype == MV_BF16 && C == 128 && K == 512 && (N2 == 128 || N2 == 256) && chain_l2_m_ok(M)) || get_flag("no_chain") ||
        get_flag("no_chain_res") || get_flag("no_chain_l2"))
        return 0;
    if (sub == 0) return 1;
    return sub == 2 && H % 2 == 0 && W % 2 == 0 && N * (H / 2) * (W / 2) * K * 2 < (1LL << 31) && !get_flag("no_chain_sub");
}

int chain_l2_res_launch(const void* t2, const void* residual, const void* wfrag, const void* shifts, void* y, void* t1, int N, int H,
                        int W, int N2, int sub, hipStream_t st) {
    ChainL2P p;
    p.xa = (const bf16_t*)t2; p.xb = nullptr; p.res = (const bf16_t*)residual; p.wf = (const bf16_t*)wfrag;
    p.sh = (const unsigned*)shifts; p.y = (bf16_t*)y; p.t1 = (bf16_t*)t1;
    p.subH = H; p.subW = W;
    const long long M = (long long)N * H * W;
    if (N2 == 256) {
        if (sub) {
            set_kernel_name("chain_l2_exit_bf16_128_512_256_ysub2");
            return chain_l2_go<128, 0, true, 256, true, 4, 2, 6>(p, M, st);
        }
        set_kernel_name("chain_l2_exit_bf16_128_512_256");
        return chain_l2_go<128, 0, true, 256, false, 4, 2, 6>(p, M, st);
    }
    if (sub) {
        set_kernel_name("chain_l2_res_bf16_128_512_128_ysub2");
        return chain_l2_go<128, 0, true, 128, true, 8, 2, 6>(p, M, st);
    }
    set_kernel_name("chain_l2_res_bf16_128_512_128");
    return chain_l2_go<128, 0, true, 128, false, 8, 2, 6>(p, M, st);
}

int chain_l2_dual_supported(long long M, int C1, int C2, int K, int N2, int dtype) {
    return dtype == MV_BF16 && C1 == 128 && C2 == 256 && K == 512 && N2 == 128 && chain_l2_m_ok(M) && !get_flag("no_chain") &&
           !get_flag("no_chain_l2");
}

int chain_l2_dual_launch(const void* t2, const void* x, const void* wfrag, const void* shifts, void* y, void* t1, long long M,
                         hipStream_t st) {
    ChainL2P p;
    p.xa = (const bf16_t*)t2; p.xb = (const bf16_t*)x; p.res = nullptr; p.wf = (const bf16_t*)wfrag;
    p.sh = (const unsigned*)shifts; p.y = (bf16_t*)y; p.t1 = (bf16_t*)t1;
    p.subH = 0; p.subW = 0;
    set_kernel_name("chain_l2_entry_bf16_128+256_512_128");
    return chain_l2_go<128, 256, false, 128, false, 4, 2, 6>(p, M, st);
}

}  // namespace mv
