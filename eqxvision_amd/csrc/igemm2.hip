// Deep-pipelined implicit GEMM for the compute-bound layers (3x3 convolutions, ViT / Swin Linears),
// gfx950.  Same math, operand layouts and epilogue as igemm.hip; what changes is the pipeline:
//
//  * 512 threads = 8 waves (2 per SIMD), block tile 256 pixels x 128 (or 64) channels, k-tile 64.
//  * an S = 3 stage LDS ring filled by LDS-DMA (`global_load_lds_dwordx4`): the DMA for k-tile t+2 is
//    issued while tile t is being multiplied, so ~2 tile-times (~2000 cycles) of HBM/L2 latency are
//    covered.  The 128^2 kernel prefetched ONE tile ahead (~500 cycles): measured 25% MFMA utilisation.
//  * hipcc cannot express this: it makes every ds_read that follows an LDS-DMA wait for vmcnt(0) and
//    drains the queue at __syncthreads().  So the steady state uses
//        - `s_waitcnt vmcnt(N)` with a COUNTED N (inline asm): only the oldest tile has to have landed,
//        - raw `s_barrier`,
//        - inline-asm `ds_read_b128` for the MFMA fragments (invisible to the compiler's LDS-DMA alias
//          check) with hand-counted `lgkmcnt`, software-pipelined one k16-step ahead of the MFMAs;
//          every wait names the fragment registers it guards as "+v" operands so no MFMA can be
//          scheduled above it (cdna_hip_programming.md section 5.7).
//  * vmcnt counts in issue order, so the residual / scale / shift prefetch issued before the ring is
//    always older than any DMA and never disturbs the counts; there are no stores before the epilogue.
#include "conv_launchers.h"
#include "igemm_pipe.h"

namespace mv {

// WM x WN waves (= 8), each TM x TN tiles of 32x32.  BM = 32*TM*WM pixels, BN = 32*TN*WN channels (TN*32 = 64).
// NST = LDS ring depth (3 for the 256x128 / 256x64 tiles, 2 for 256x256 whose k-tile alone lasts ~2000
// cycles); RESPF = prefetch the residual rows before the main loop (needs TM*4 16-byte registers).
// DUAL: two reduction sources that add into one output -- a dense pointwise layer on x (C channels) and a strided
// pointwise layer on x2 (C2 channels at pixel stride s2): a ResNet stage's first bottleneck, conv3 + the downsample conv
// (resnet.py:144-162, 295-303).  The k-tiles walk x's channels, then x2's; weight rows are [C | C2] long.
template <int WM, int WN, int TM, int TN, int NST, bool RESPF, typename OutT, bool DUAL = false>
__global__ __launch_bounds__(512) void igemm2_kernel(const Igemm2P p) {
    constexpr int BM = 32 * TM * WM, BN = 32 * TN * WN;
    constexpr int ROWB = 128;
    constexpr int XI = BM / 64, WI = BN / 64;            // DMA instructions per thread per k-tile (8 waves x 8 rows)
    constexpr int L = XI + WI;
    constexpr int STAGE = (BM + BN) * ROWB;
    constexpr int EPITCH = 64 * 4 + 16;
    static_assert(WM * WN == 8 && TN == 2, "8 waves; a wave covers 64 channels (one 128-byte output line)");
    static_assert(8 * 32 * EPITCH <= NST * STAGE, "epilogue patches must fit");
    static_assert((NST - 1) * L <= 63, "vmcnt immediate");
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    long long pt0 = 0, pt1 = 0, pt2 = 0;
    if (p.prof) pt0 = wall_clock64();
    const int t = xcd_remap(blockIdx.x, p.tiles_m * p.tiles_n);
    int tile_m, tile_n;
    tile_coords(t, p.tiles_m, p.tiles_n, tile_m, tile_n);
    const int m0 = tile_m * BM, n0 = tile_n * BN;

    // ---------------- DMA addressing -------------------------------------------------------------------
    // Per staged row: ONE 64-bit element offset of the tap-(0,0), channel-0 source and a bit mask of the
    // filter taps that fall inside the image, both computed once.  Per k-tile the source of a lane is
    // then `valid_bit ? x + base + tapdelta : zero_page` with a wave-uniform tapdelta: ~7 VALU per DMA
    // instead of re-deriving (hi, wi), two range checks and a 64-bit multiply chain every k-tile.
    const int srow = lane >> 3;
    const int chunk = (lane & 7) ^ ((4 * wave + (lane >> 4)) & 7);
    const int cpt = p.C >> 6;
    const int nk = DUAL ? ((p.C + p.C2) >> 6) : p.R * p.S * cpt;
    const long long wrow_stride = DUAL ? (long long)(p.C + p.C2) : (long long)p.R * p.S * p.C;
    const bool dense1x1 = p.R == 1 && p.S == 1 && p.sh == 1 && p.sw == 1 && p.ph == 0 && p.pw == 0;   // block-uniform
    long long xbase[XI];
    unsigned vlo[XI], vhi[XI];
    // Row m -> (image b, output row ho, output column wo).  The block's first row is decomposed once with integer
    // divisions (block-uniform); every staged row is that plus an offset < 256 + Wo, small enough for an exact
    // float-reciprocal division (one multiply + a +-1 correction).  Four full division chains per lane cost 2.4 us of
    // prologue per tile on the 3x3 layers (phase stamps: 3.6 us against 1.2 us for a dense layer).
    const int b0 = m0 / (p.Ho * p.Wo), rem0 = m0 - b0 * (p.Ho * p.Wo);
    const int ho0 = rem0 / p.Wo, wo0 = rem0 - ho0 * p.Wo;
    const float inv_wo = 1.0f / (float)p.Wo, inv_ho = 1.0f / (float)p.Ho;
    auto small_div = [](int v, int d, float inv, int& q, int& r) {      // 0 <= v < 2^22
        q = (int)((float)v * inv);
        r = v - q * d;
        if (r >= d) { ++q; r -= d; }
        if (r < 0) { --q; r += d; }
    };
    long long xbase2[DUAL ? XI : 1];
#pragma unroll
    for (int j = 0; j < XI; ++j) {
        const int roff = 8 * (wave + 8 * j) + srow;
        const int m = m0 + roff;
        const bool valid = m < p.M;
        if (dense1x1) {                                   // a Linear: row m is pixel m, one tap, no division at all
            xbase[j] = (long long)m * p.C + chunk * 8;
            vlo[j] = valid ? 1u : 0u;
            vhi[j] = 0u;
            continue;
        }
        int qw, wo, qh, ho;
        small_div(wo0 + roff, p.Wo, inv_wo, qw, wo);
        small_div(ho0 + qw, p.Ho, inv_ho, qh, ho);
        const int b = b0 + qh;
        const int hi0 = ho * p.sh - p.ph, wi0 = wo * p.sw - p.pw;
        xbase[j] = (long long)((b * p.H + hi0) * p.W + wi0) * p.C + chunk * 8;    // pixel index fits 32 bits (N*H*W < 2^31)
        if constexpr (DUAL) xbase2[j] = (long long)((b * p.H2 + ho * p.s2) * p.W2 + wo * p.s2) * p.C2 + chunk * 8;
        unsigned long long mask = 0;
        if constexpr (DUAL) {
            mask = valid ? 3ull : 0ull;                   // both sources exist for every output pixel
        } else if (valid) {
            if (p.R == 3 && p.S == 3) {                    // the common case, branch-free: 3 + 3 range checks
                const unsigned W_ = (unsigned)p.W, H_ = (unsigned)p.H;
                const unsigned cols = ((unsigned)wi0 < W_ ? 1u : 0u) | ((unsigned)(wi0 + p.dw) < W_ ? 2u : 0u) |
                                      ((unsigned)(wi0 + 2 * p.dw) < W_ ? 4u : 0u);
                mask = ((unsigned)hi0 < H_ ? cols : 0u) | ((unsigned)(hi0 + p.dh) < H_ ? cols << 3 : 0u) |
                       ((unsigned)(hi0 + 2 * p.dh) < H_ ? cols << 6 : 0u);
            } else if (p.R * p.S <= 32) {                  // rows and columns are independent: R + S range checks, not R * S
                unsigned cols = 0;
                for (int s = 0; s < p.S; ++s)
                    if ((unsigned)(wi0 + s * p.dw) < (unsigned)p.W) cols |= 1u << s;
                unsigned m32 = 0;
                for (int r = 0; r < p.R; ++r)
                    if ((unsigned)(hi0 + r * p.dh) < (unsigned)p.H) m32 |= cols << (r * p.S);
                mask = m32;
            } else {
                for (int r = 0; r < p.R; ++r) {
                    const int hi = hi0 + r * p.dh;
                    if ((unsigned)hi >= (unsigned)p.H) continue;
                    for (int s = 0; s < p.S; ++s) {
                        const int wi = wi0 + s * p.dw;
                        if ((unsigned)wi < (unsigned)p.W) mask |= 1ull << (r * p.S + s);
                    }
                }
            }
        }
        vlo[j] = (unsigned)mask;
        vhi[j] = (unsigned)(mask >> 32);
    }
    long long woff[WI];
#pragma unroll
    for (int j = 0; j < WI; ++j) {
        const int n = n0 + 8 * (wave + 8 * j) + srow;
        woff[j] = n < p.K ? (long long)n * wrow_stride + chunk * 8 : -1;
    }
    // one DMA piece: piece q < XI stages 8 pixel rows of the x tile, q >= XI stages 8 weight rows
    auto stage_piece = [&](int q, int buf, int r, int s, int c0) {
        char* xs = smem + buf * STAGE;
        char* ws = xs + BM * ROWB;
        const int tp = r * p.S + s;                                          // wave-uniform
        if (q < XI) {
            const unsigned bits = tp < 32 ? vlo[q] : vhi[q];
            const bool ok = (bits >> (tp & 31)) & 1u;
            const bf16_t* src;
            if constexpr (DUAL) {                          // "tap" s = the source: 0 = x (dense), 1 = x2 (strided)
                src = ok ? (s == 0 ? p.x + xbase[q] + c0 : p.x2 + xbase2[q] + c0) : p.zero;
            } else {
                const long long tapdelta = ((long long)(r * p.dh) * p.W + s * p.dw) * p.C + c0;
                src = ok ? p.x + tapdelta + xbase[q] : p.zero;
            }
            glds16(src, xs + 8 * (wave + 8 * q) * ROWB);
        } else {
            const int j = q - XI;
            const int tapoff = tp * p.C + c0;                // DUAL: tp = s in {0, 1}: source 1's weights start at column C
            const bf16_t* src = woff[j] >= 0 ? p.w + woff[j] + tapoff : p.zero;
            glds16(src, ws + 8 * (wave + 8 * j) * ROWB);
        }
    };
    auto stage = [&](int buf, int r, int s, int c0) {
#pragma unroll
        for (int q = 0; q < L; ++q) stage_piece(q, buf, r, s, c0);
    };

    // ---------------- fragment addressing ------------------------------------------------------------
    const int wm = wave % WM, wn = wave / WM;
    const int fr = lane & 31, fh = lane >> 5, swz = (fr >> 1) & 7;
    const int xrow0 = wm * (32 * TM), wrow0 = wn * (32 * TN);
    const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) char*)smem;
    unsigned xaddr[4], waddr[4];     // per k16-step: byte address of my 16-byte fragment in stage 0
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
        const unsigned ko = (unsigned)(((2 * kk + fh) ^ swz) << 4);
        xaddr[kk] = lds0 + (xrow0 + fr) * ROWB + ko;
        waddr[kk] = lds0 + BM * ROWB + (wrow0 + fr) * ROWB + ko;
    }

    // ---------------- epilogue constants + residual prefetch (older than every DMA) --------------------
    const OutT* res = (const OutT*)p.residual;
    ScaleShift8 ss;
    ss.load(p.scale, p.shift, n0 + wrow0 + (lane & 7) * 8, p.K);
    // Residual rows are fetched in the MIDDLE of the reduction (end of iteration `jres`), not before it: issued up
    // front they are older than the first k-tile, whose counted wait then sits behind 64-128 KB of residual traffic
    // per block (measured: 5.8 us of prologue instead of 1.8 on the ViT projections).  vmcnt retires in issue
    // order, so for the NST-1 iterations that follow the issue the counted wait allows RL more operations in flight.
    constexpr int RL = TM * 4 * (sizeof(OutT) == 4 ? 2 : 1);
    static_assert(!RESPF || (NST - 2) * L + RL <= 63, "vmcnt immediate");
    R8<OutT> rres[RESPF ? TM : 1][4];
    auto fetch_residual = [&]() {
        asm volatile("" ::: "memory");                     // keep the loads at this point of the issue order
#pragma unroll
        for (int b = 0; b < TM; ++b)
#pragma unroll
            for (int pass = 0; pass < 4; ++pass) {
                const int m = m0 + xrow0 + b * 32 + pass * 8 + (lane >> 3);
                const int n = n0 + wrow0 + (lane & 7) * 8;
                const bool ok = m < p.M && n < p.K;
                rres[RESPF ? b : 0][pass].load(res + (ok ? (long long)m * p.K + n : 0));
            }
        asm volatile("" ::: "memory");
    };

    f32x16 acc[TN][TM];
#pragma unroll
    for (int a = 0; a < TN; ++a)
#pragma unroll
        for (int b = 0; b < TM; ++b)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[a][b][e] = 0.f;

    // ---------------- ring prologue: tiles 0 .. NST-2 ----------------------------------------------------
    int r = 0, s = 0, c0 = 0;
    auto advance = [&]() {
        c0 += 64;
        if (c0 == ((DUAL && s == 1) ? p.C2 : p.C)) {
            c0 = 0;
            if (++s == p.S) {
                s = 0;
                ++r;
            }
        }
    };
    int issued = 0;
#pragma unroll
    for (int i = 0; i < NST - 1; ++i) {
        if (issued < nk) {
            stage(i, r, s, c0);
            advance();
            ++issued;
        }
    }

    if (p.prof) pt1 = wall_clock64();
    // ---------------- main loop ---------------------------------------------------------------------------
    int cur = 0;
    int raised = 0;                                        // iterations left whose wait must let the residual rows fly
    const int jres = p.dbg ? -1 : (nk - 1) >> 1;
    if (RESPF && res && p.dbg) fetch_residual();          // A/B: the old up-front fetch
    for (int it = 0; it < nk; ++it) {
        // tile `it` must have landed; younger tiles (at most NST-2) may stay in flight
        const int younger = issued - it - 1;
        if (NST > 2 && younger >= NST - 2) {
            if (RESPF && raised > 0) wait_vm<(NST > 2 ? (NST - 2) * L + (RESPF ? RL : 0) : 0)>();
            else wait_vm<(NST > 2 ? (NST - 2) * L : 0)>();
        } else {
            wait_vm<0>();
        }
        if (RESPF && raised > 0) --raised;
        __builtin_amdgcn_s_barrier();
        // Refill the stage everyone just left with tile it+NST-1.  The L DMA pieces are spread over the four
        // k16-steps below (a quarter per step, between the fragment reads and the MFMAs) so their address
        // VALU/SALU work hides under MFMA execution instead of forming a block of its own after the barrier.
        // vmcnt accounting is unchanged: they are still the newest L operations at the next iteration's wait.
        const bool refill = issued < nk;
        int rbuf = cur + NST - 1;
        if (rbuf >= NST) rbuf -= NST;
        const unsigned sb = (unsigned)(cur * STAGE);
        u32x4 af[2][TN], bfm[2][TM];
        auto read_step = [&](int set, int kk) {
            lds_read16<0>(af[set][0], waddr[kk] + sb);
            lds_read16<32 * ROWB>(af[set][1], waddr[kk] + sb);
            lds_read16<0>(bfm[set][0], xaddr[kk] + sb);
            if constexpr (TM >= 2) lds_read16<32 * ROWB>(bfm[set][1], xaddr[kk] + sb);
            if constexpr (TM >= 3) lds_read16<64 * ROWB>(bfm[set][2], xaddr[kk] + sb);
            if constexpr (TM >= 4) lds_read16<96 * ROWB>(bfm[set][3], xaddr[kk] + sb);
        };
        auto wait_step = [&](int set, bool last) {
            // the TN+TM reads of this step are done once at most TN+TM younger ones remain in flight;
            // naming the fragments as "+v" operands pins every consumer MFMA below the wait
            if constexpr (TM == 1) {
                if (last) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(af[set][0]), "+v"(af[set][1]), "+v"(bfm[set][0]));
                else asm volatile("s_waitcnt lgkmcnt(3)" : "+v"(af[set][0]), "+v"(af[set][1]), "+v"(bfm[set][0]));
            } else if constexpr (TM == 2) {
                if (last) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(af[set][0]), "+v"(af[set][1]), "+v"(bfm[set][0]), "+v"(bfm[set][1]));
                else asm volatile("s_waitcnt lgkmcnt(4)" : "+v"(af[set][0]), "+v"(af[set][1]), "+v"(bfm[set][0]), "+v"(bfm[set][1]));
            } else {
                static_assert(TM == 4, "TM in {1,2,4}");
                if (last) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(af[set][0]), "+v"(af[set][1]), "+v"(bfm[set][0]), "+v"(bfm[set][1]), "+v"(bfm[set][2]), "+v"(bfm[set][3]));
                else asm volatile("s_waitcnt lgkmcnt(6)" : "+v"(af[set][0]), "+v"(af[set][1]), "+v"(bfm[set][0]), "+v"(bfm[set][1]), "+v"(bfm[set][2]), "+v"(bfm[set][3]));
            }
        };
        read_step(0, 0);
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            const int cs = kk & 1, ns = cs ^ 1;
            if (kk < 3) read_step(ns, kk + 1);
            // a quarter of the refill DMA (address VALU + issue) rides in the shadow of this step's MFMAs
            if (refill) {
#pragma unroll
                for (int q = (kk * L) / 4; q < ((kk + 1) * L) / 4; ++q) stage_piece(q, rbuf, r, s, c0);
            }
            wait_step(cs, kk == 3);
#pragma unroll
            for (int a = 0; a < TN; ++a)
#pragma unroll
                for (int b = 0; b < TM; ++b)
                    acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, af[cs][a]),
                                                                        __builtin_bit_cast(bf16x8, bfm[cs][b]),
                                                                        acc[a][b], 0, 0, 0);
        }
        if (refill) {
            advance();
            ++issued;
        }
        if (RESPF && res && it == jres) {
            fetch_residual();
            raised = NST - 1;
        }
        if (++cur == NST) cur = 0;
    }

    // ---------------- epilogue (as igemm.hip: LDS transpose, full-line stores) ------------------------------
    __syncthreads();
    if (p.prof) pt2 = wall_clock64();
    char* ep = smem + wave * (32 * EPITCH);
    OutT* y = (OutT*)p.y;
    if constexpr (!RESPF && TN == 2) {    // branch-free buffer loads / stores (igemm_pipe.h), residual rows one pixel tile ahead
        epilogue_rows<OutT, false, TM, EPITCH>(p, ep, acc, ss, res, true, m0 + xrow0, n0 + wrow0, lane);
    } else
#pragma unroll
    for (int b = 0; b < TM; ++b) {
        R8<OutT> late[4];                 // no prefetch: fetch this pixel tile's 4 residual rows together
        if (!RESPF && res) {
#pragma unroll
            for (int pass = 0; pass < 4; ++pass) {
                const int m = m0 + xrow0 + b * 32 + pass * 8 + (lane >> 3);
                const int n = n0 + wrow0 + (lane & 7) * 8;
                const bool ok = m < p.M && n < p.K;
                late[pass].load(res + (ok ? (long long)m * p.K + n : 0));
            }
        }
#pragma unroll
        for (int a = 0; a < TN; ++a)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int nl = a * 32 + 8 * g + 4 * fh;
                *(float4*)(ep + fr * EPITCH + nl * 4) = make_float4(acc[a][b][4 * g + 0], acc[a][b][4 * g + 1],
                                                                     acc[a][b][4 * g + 2], acc[a][b][4 * g + 3]);
            }
#pragma unroll
        for (int pass = 0; pass < 4; ++pass) {
            const int row = pass * 8 + (lane >> 3), c8 = lane & 7;
            const int m = m0 + xrow0 + b * 32 + row;
            const int n = n0 + wrow0 + c8 * 8;
            const float4 lo = *(const float4*)(ep + row * EPITCH + c8 * 32);
            const float4 hi = *(const float4*)(ep + row * EPITCH + c8 * 32 + 16);
            if (m < p.M && n < p.K) {
                float v[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
                ss.apply(v);
                if (res) {
                    if constexpr (RESPF) rres[b][pass].add_to(v);
                    else late[pass].add_to(v);
                }
                if (p.act == MV_ACT_RELU) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) v[e] = fmaxf(v[e], 0.f);
                } else if (p.act == MV_ACT_GELU_TANH) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) v[e] = gelu_tanh_f(v[e]);
                }
                long long off = (long long)m * p.K + n;
                if (p.tok > 0) {          // 64 channels = one head = one 128-byte line: same store width, new home
                    const int bi = m / p.tok, ti = m - bi * p.tok;
                    off = (((long long)bi * (p.K >> 6) + (n >> 6)) * p.tok + ti) * 64 + (n & 63);
                }
                Out8<OutT>::st(y + off, v);
            }
        }
    }
    if (p.prof && tid == 0) {
        long long* o = p.prof + 4ll * blockIdx.x;
        o[0] = pt0; o[1] = pt1; o[2] = pt2; o[3] = wall_clock64();
    }
}

template <int WM, int WN, int TM, int TN, int NST, bool RESPF>
static int launch2(Igemm2P& p, bool out_f32, hipStream_t st) {
    constexpr int BM = 32 * TM * WM, BN = 32 * TN * WN;
    constexpr int SMEM = NST * (BM + BN) * 128;
    p.tiles_m = (p.M + BM - 1) / BM;
    p.tiles_n = (p.K + BN - 1) / BN;
    dim3 grid((unsigned)(p.tiles_m * p.tiles_n)), block(512);
#define GO(OT)                                                                                                   \
    do {                                                                                                         \
        auto kern = igemm2_kernel<WM, WN, TM, TN, NST, RESPF, OT>;                                               \
        MV_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, SMEM));        \
        hipLaunchKernelGGL(kern, grid, block, SMEM, st, p);                                                      \
    } while (0)
    if (out_f32) GO(float); else GO(bf16_t);
#undef GO
    MV_LAUNCH_CHECK();
    return MV_OK;
}

// y[N,Ho,Wo,K] = act(scale[k] * (x[N,Ho,Wo,C1] . w[k, 0:C1] + x2[N, s2*ho, s2*wo, C2] . w[k, C1:C1+C2]) + shift[k])
int igemm2_dual_launch(const void* x, const void* x2, const void* w, const float* scale, const float* shift, void* y, int N,
                       int Ho, int Wo, int C1, int H2, int W2, int C2, int s2, int K, int act, int tile, hipStream_t st) {
    Igemm2P p;
    p.tok = 0;
    p.dbg = 0;
    p.prof = nullptr;
    p.x = (const bf16_t*)x; p.w = (const bf16_t*)w; p.scale = scale; p.shift = shift; p.residual = nullptr; p.y = y;
    p.x2 = (const bf16_t*)x2; p.C2 = C2; p.H2 = H2; p.W2 = W2; p.s2 = s2;
    p.zero = (const bf16_t*)zero_page(st);
    if (!p.zero) {
        set_error("igemm2: zero page allocation failed");
        return MV_E_OOM;
    }
    if ((long long)N * H2 * W2 >= (1LL << 31) - (1LL << 20)) {
        set_error("igemm2 dual: %lld input pixels do not fit the 32-bit pixel index", (long long)N * H2 * W2);
        return MV_E_UNSUPPORTED;
    }
    p.N = N; p.H = Ho; p.W = Wo; p.C = C1; p.K = K; p.R = 1; p.S = 2;       // S = 2 "taps" = the two sources
    p.Ho = Ho; p.Wo = Wo;
    p.sh = 1; p.sw = 1; p.ph = 0; p.pw = 0; p.dh = 1; p.dw = 1;
    p.M = (int)((long long)N * Ho * Wo);
    p.act = act;
    p.tiles_m = (p.M + 255) / 256;
    if (tile == 3) {                                        // (route.h: route_conv1x1_dual)
        constexpr int SMEM = 2 * (256 + 256) * 128;
        p.tiles_n = (K + 255) / 256;
        auto kern = igemm2_kernel<2, 4, 4, 2, 2, false, bf16_t, true>;
        MV_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, SMEM));
        hipLaunchKernelGGL(kern, dim3((unsigned)(p.tiles_m * p.tiles_n)), dim3(512), SMEM, st, p);
    } else {
        constexpr int SMEM = 3 * (256 + 128) * 128;
        p.tiles_n = (K + 127) / 128;
        auto kern = igemm2_kernel<4, 2, 2, 2, 3, true, bf16_t, true>;
        MV_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, SMEM));
        hipLaunchKernelGGL(kern, dim3((unsigned)(p.tiles_m * p.tiles_n)), dim3(512), SMEM, st, p);
    }
    MV_LAUNCH_CHECK();
    return MV_OK;
}

// block tile igemm2_launch picks for (M rows, K output channels) when it is not told one
static int igemm2_tile_shape(long long M, int K, int* bm, int* bn) {
    const int tile = igemm2_tile_rule(M, K, get_flag("igemm2_tile"));
    *bm = 256;
    *bn = tile == 1 ? 64 : (tile == 3 ? 256 : 128);
    return tile;
}

int igemm2_launch(const void* x, const void* w, const float* scale, const float* shift, const void* residual, void* y,
                  const ConvShape& s, int tile, int tok, hipStream_t st) {
    Igemm2P p;
    p.tok = tok;
    p.x2 = nullptr; p.C2 = 0; p.H2 = 0; p.W2 = 0; p.s2 = 1;
    p.dbg = 0;
#ifdef MV_I8_PROF      // debug builds only: a raw device pointer taken from flags must never reach a captured graph
    p.prof = (long long*)(((unsigned long long)(unsigned)get_flag("prof_hi") << 32) | (unsigned)get_flag("prof_lo"));
#else
    p.prof = nullptr;
#endif
    p.x = (const bf16_t*)x; p.w = (const bf16_t*)w; p.scale = scale; p.shift = shift; p.residual = residual; p.y = y;
    const int rc = fill_geometry(p, s, "igemm2", true, st);
    if (rc != MV_OK) return rc;
    const bool out_f32 = s.out_dtype == MV_F32;
    int bm_, bn_;
    if (tile == 0) tile = igemm2_tile_shape(s.M(), s.K, &bm_, &bn_);   // 1 = 256x64, 2 = 256x128, 3 = 256x256
    if (tile == 1) return launch2<8, 1, 1, 2, 3, true>(p, out_f32, st);
    if (tile == 3) return launch2<2, 4, 4, 2, 2, false>(p, out_f32, st);
    return launch2<4, 2, 2, 2, 3, true>(p, out_f32, st);
}

}  // namespace mv
