// Ping-pong implicit GEMM with 512-cycle phases, 256 pixels x 256 channels x 64 (k) per step, gfx950.
//
// The matrix pipe of a SIMD is shared by the two waves a 512-thread block puts on it.  igemm2 lets both waves run
// the same schedule (reads, DMA issue and MFMAs interleaved in each wave); here the two waves of a SIMD never do the
// same thing at the same time:
//
//   * the 8 waves form two groups of four (group g = wave / 4 owns pixel rows 128 g .. 128 g + 127 of the tile, its
//     four waves 64 channels each), one wave of each group per SIMD; a wave's accumulator is 128 x 64 (8 MFMA tiles
//     of 32 x 32 = 128 registers);
//   * a k-tile of 64 is TWO phases, each a LOAD half and an MFMA half separated by raw `s_barrier`s:
//         phase 1  LOAD: 16 ds_read_b128 (weights 64 x 64, pixels 0..63 x 64)   MFMA: 16 x v_mfma_f32_32x32x16_bf16
//         phase 2  LOAD:  8 ds_read_b128 (pixels 64..127 x 64)                  MFMA: 16 x ...
//     so an MFMA half is 512 cycles of back-to-back matrix work (round 1's ping-pong kernel had 256-cycle phases: twice the
//     barriers per FLOP); group 1 runs one barrier behind group 0, so on every SIMD one wave is in its MFMA half while its partner
//     is in its LOAD half;
//   * LDS holds two k-tiles (2 x 64 KB), each as three DMA units that are re-staged as soon as their last reader is
//     done, not when the whole tile is: W (256 x 64, read in phase 1), Xtop (the 2 x 64 phase-1 pixel rows) and Xbot
//     (the phase-2 rows).  Per thread a k-tile is 8 LDS-DMA instructions (16 bytes per lane), spread 3 / 5 over the two
//     LOAD halves so that both stay shorter than the partner's 512-cycle MFMA half.  Every wait is a counted
//     `s_waitcnt vmcnt(8 | 7)`: one whole k-tile stays in flight across the barriers.
//   * the DMA is `buffer_load_dwordx4 ... offen lds`: the per-lane part of an address (row base) is a 32-bit VGPR
//     offset computed ONCE, the per-k-tile part (filter tap, channel block) is a scalar offset, and rows that fall in
//     the zero padding / beyond M or K get an out-of-range offset -- the buffer unit then writes zeros, so there is
//     no zero page, no 64-bit pointer select and ~3 VALU per piece instead of ~7 (igemm2);
//   * LDS rows are 128 bytes, lane-linear for the DMA; the 16-byte chunk a lane fetches is XOR-swizzled on the
//     SOURCE side (chunk ^ ((row >> 1) & 7)) and the fragment reads apply the same XOR (conflict-free ds_read_b128).
//
// Operands, accumulator layout and epilogue are igemm2's (A = weights, B = pixels: a lane ends with 4 consecutive
// channels of one pixel; wave-private LDS transpose, full 128-byte line stores; scale/shift, residual, activation,
// head-major token output).  DUAL: a second reduction source x2 (pointwise, pixel stride s2) appended to the
// reduction -- ResNet conv3 + downsample conv (resnet.py:144-162, 295-303), or x2 = x with the low halves of split
// bf16 weights for the precision-critical Linears.
#include <type_traits>

#include "conv_launchers.h"
#include "igemm_pipe.h"

namespace mv {

namespace {

constexpr unsigned OOB = 0x80000000u;          // >= num_records of every descriptor: the DMA writes zeros

// Device status word (mv_device_status): bit 0 = a split-K block gave up waiting for its partner's partial tile; bit 1 = a counted
// pixel of mv_softmax_xent_map_f32 had a label outside [0, C) (seg_bwd.hip, through device_status_word()).  A kernel that
// finds its hand-over broken RECORDS it here and finishes with what it has -- it does not trap: a trap is a sticky
// hipErrorLaunchFailure that poisons the whole context (an in-flight graph replay, other streams) and surfaces at an unrelated
// call (advisor, round 5).  The host reads the word at its own synchronisation points and fails with a clear message.
__device__ unsigned g_dev_status = 0;
constexpr int LDS_W = 0, LDS_XT = 65536, LDS_XB = 98304;   // unit bases of buffer 0; buffer 1: W +32768, XT/XB +16384
constexpr int LDS_TOTAL = 131072;
// LayerNorm fold, consumer side (LNF 2): behind the operand buffers the 256 rows' statistics pieces as the producers wrote them
// (one piece of 256 x (sum, m2) = 2 KB per 256 columns of the row, up to 3) and the finalised 256 x (-mean * rstd, rstd);
// producer side: behind the epilogue patches 256 rows x 4 waves x (sum, m2) and 512 dummy bytes per wave
constexpr int LDS_LNP = LDS_TOTAL, LN_MAXP = 3, LDS_LNS = LDS_LNP + LN_MAXP * 2048, LDS_TOTAL_LN = LDS_LNS + 2048;
constexpr int LDS_LN_SLOTS = 8 * 32 * (64 * 4 + 16), LDS_LN_DUMMY = LDS_LN_SLOTS + 256 * 32;
static_assert(LDS_LN_DUMMY + 8 * 512 <= LDS_TOTAL, "producer statistics slots");

template <int LOFF>
__device__ __forceinline__ void dma16(unsigned ldsw, unsigned voff, const u32x4& rsrc, unsigned soff) {
    asm volatile("s_add_u32 m0, %0, %4\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds"
                 :
                 : "s"(ldsw), "v"(voff), "s"(rsrc), "s"(soff), "n"(LOFF)
                 : "memory", "scc");
}

template <int LOFF>
__device__ __forceinline__ void dma4(unsigned ldsw, unsigned voff, const u32x4& rsrc, unsigned soff) {      // one dword per lane
    asm volatile("s_add_u32 m0, %0, %4\n\tbuffer_load_dword %1, %2, %3 offen lds"
                 :
                 : "s"(ldsw), "v"(voff), "s"(rsrc), "s"(soff), "n"(LOFF)
                 : "memory", "scc");
}

__device__ __forceinline__ u32x4 make_rsrc(const void* base) {
    const unsigned long long b = (unsigned long long)base;
    u32x4 r;
    r[0] = __builtin_amdgcn_readfirstlane((unsigned)b);
    r[1] = __builtin_amdgcn_readfirstlane((unsigned)(b >> 32) & 0xffffu);      // stride 0: raw buffer
    r[2] = OOB;                                                                 // num_records (bytes)
    r[3] = 0x00020000u;                                                         // gfx9 raw-buffer data format
    return r;
}

template <int N> __device__ __forceinline__ void wait_vm_lgkm0() {
    asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(N) : "memory");
}

}  // namespace

struct TapState {          // the k-tile a DMA unit is being staged for: scalar source offsets of both operands
    int r, s, c0;          // filter tap and first channel
    unsigned xoff;         // byte offset of (tap, c0) from the x descriptor base
    unsigned woff;         // byte offset of the k-tile inside a weight row
    unsigned bit;          // 1 << tap index (which bit of a row's tap mask decides valid / zero padding)
};

__device__ __forceinline__ TapState tap_first() {
    TapState s;
    s.r = 0; s.s = 0; s.c0 = 0; s.xoff = 0; s.woff = 0; s.bit = 1u;
    return s;
}

// -> state of k-tile `tile` (called with consecutive tiles); nk1 = k-tiles of the first source
template <bool DUAL> __device__ __forceinline__ void tap_next(const Igemm2P& p, TapState& s, int tile, int nk1) {
    s.woff += 128u;
    if (DUAL && tile >= nk1) {                   // second source: one "tap", channels (tile - nk1) * 64
        s.xoff = 128u * (unsigned)(tile - nk1);
        return;
    }
    s.c0 += 64;
    if (s.c0 == p.C) {
        s.c0 = 0;
        if (++s.s == p.S) { s.s = 0; ++s.r; }
        s.bit <<= 1;
    }
    s.xoff = 2u * (unsigned)(((s.r * p.dh) * p.W + s.s * p.dw) * p.C + s.c0);
}

// -> state of k-tile `tile` from scratch (a split-K block starts in the middle of the reduction)
template <bool DUAL> __device__ __forceinline__ TapState tap_at(const Igemm2P& p, int tile, int nk1) {
    TapState s = tap_first();
    s.woff = 128u * (unsigned)tile;
    if (DUAL && tile >= nk1) {
        s.xoff = 128u * (unsigned)(tile - nk1);
        return s;
    }
    const int cpt = p.C >> 6, tap = tile / cpt;
    s.c0 = (tile - tap * cpt) * 64;
    s.r = tap / p.S;
    s.s = tap - s.r * p.S;
    s.bit = 1u << tap;
    s.xoff = 2u * (unsigned)(((s.r * p.dh) * p.W + s.s * p.dw) * p.C + s.c0);
    return s;
}

// Per-lane DMA source of one staged pixel row: byte offset of its tap-(0,0) / channel-0 element (+ the lane's swizzled
// 16-byte chunk) from the x descriptor base, the bit mask of the filter taps that fall inside the image, and (DUAL) the
// offset of the same output pixel in the second, strided source.  Block-uniform part (b0, ho0, wo0) done once by the caller.
struct RowBase {
    int ho0, wo0, b0;
    float inv_wo, inv_ho;
    unsigned padb;
    bool dense1x1;
};
__device__ __forceinline__ RowBase row_base(const Igemm2P& p, int m0) {
    RowBase rb;
    rb.b0 = m0 / (p.Ho * p.Wo);
    const int rem0 = m0 - rb.b0 * (p.Ho * p.Wo);
    rb.ho0 = rem0 / p.Wo;
    rb.wo0 = rem0 - rb.ho0 * p.Wo;
    rb.inv_wo = 1.0f / (float)p.Wo;
    rb.inv_ho = 1.0f / (float)p.Ho;
    rb.dense1x1 = p.R == 1 && p.S == 1 && p.sh == 1 && p.sw == 1 && p.ph == 0 && p.pw == 0;   // block-uniform
    rb.padb = rb.dense1x1 ? 0u : 2u * (unsigned)((p.ph * p.W + p.pw) * p.C);                 // keeps every row base >= 0
    return rb;
}
__device__ __forceinline__ void small_div(int v, int d, float inv, int& q, int& r) {      // 0 <= v < 2^22
    q = (int)((float)v * inv);
    r = v - q * d;
    if (r >= d) { ++q; r -= d; }
    if (r < 0) { --q; r += d; }
}
template <bool DUAL>
__device__ __forceinline__ void row_setup(const Igemm2P& p, const RowBase& rb, int m0, int roff, int gch, unsigned& vo,
                                          unsigned& mask, unsigned& vo2) {
    const int m = m0 + roff;
    const bool valid = m < p.M;
    if (rb.dense1x1 && !DUAL) {
        vo = valid ? 2u * (unsigned)(m * p.C + gch * 8) : OOB;
        mask = valid ? 1u : 0u;
        return;
    }
    int qw, wo, qh, ho;
    small_div(rb.wo0 + roff, p.Wo, rb.inv_wo, qw, wo);
    small_div(rb.ho0 + qw, p.Ho, rb.inv_ho, qh, ho);
    const int b = rb.b0 + qh;
    const int hi0 = ho * p.sh - p.ph, wi0 = wo * p.sw - p.pw;
    vo = 2u * (unsigned)(((b * p.H + hi0) * p.W + wi0) * p.C + gch * 8) + rb.padb;
    if constexpr (DUAL) vo2 = valid ? 2u * (unsigned)(((b * p.H2 + ho * p.s2) * p.W2 + wo * p.s2) * p.C2 + gch * 8) : OOB;
    unsigned mk = 0;
    if (valid) {
        unsigned cols = 0;
        for (int s = 0; s < p.S; ++s)
            if ((unsigned)(wi0 + s * p.dw) < (unsigned)p.W) cols |= 1u << s;
        for (int r = 0; r < p.R; ++r)
            if ((unsigned)(hi0 + r * p.dh) < (unsigned)p.H) mk |= cols << (r * p.S);
    }
    mask = mk;
}

// LIN: a Linear layer (dense 1x1 rows, no per-channel scale, one source).  The tap masks and the scale registers go away, which
// takes the kernel from 235 to <= 224 VGPRs: two of its waves then leave 64 registers per SIMD lane free, exactly one wave of the
// 64-register streaming kernels (LayerNorm, element-wise) -- with two graph lanes those run UNDER this kernel's main loop, whose
// memory pipe is idle, instead of time-slicing the CUs with it.
//
// MODE 0: any convolution.  MODE 1 (DENSE): a dense 1x1 layer, one source -- no tap masks, the k-tile advance is two additions
// (measured on the ViT qkv shape: 114.6 -> 101.4 us, the DMA issue path loses its per-piece mask test).  MODE 2 (LIN) = DENSE
// without the per-channel scale (Linear layers).
//
// LNF (igemm_pipe.h: epilogue_rows_ln): 1 / 3 / 4 = a Linear that adds to the residual stream in front of a LayerNorm + Linear pair
// (MODE 2; 1: fp32 rows in, bf16 planes + row-statistics pieces out; 3: planes in, planes + pieces out; 4: planes in, fp32 rows out);
// 2 = the Linear behind that LayerNorm, on the un-normalised high plane (MODE 1: scale = colsum(W'), shift = b'): the pieces of its 256
// rows are DMA'd into LDS ahead of the first k-tile (older than every operand piece, so the counted waits of the main loop stand),
// finalised by 256 threads while the first k-tile is in flight.
template <typename OutT, bool DUAL, int MODE = 0, int LNF = 0>
__global__ __launch_bounds__(512) void igemm8_kernel(const Igemm2P p) {
    constexpr bool DENSE = MODE >= 1, LIN = MODE == 2;
    static_assert(!(DUAL && DENSE), "DENSE is single-source");
    static_assert(LNF == 0 || (LNF != 2 && MODE == 2) || (LNF == 2 && MODE == 1), "LayerNorm fold: producer = LIN, consumer = DENSE");
    constexpr int BM = 256, BN = 256;
    constexpr int ROWB = 128;
    constexpr int EPITCH = 64 * 4 + 16;
    static_assert(8 * 32 * EPITCH <= LDS_TOTAL, "epilogue patches must fit");
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int grp = wave >> 2, wc = wave & 3;
#ifdef MV_I8_PROF      // debug builds only (EQV_PROF=1 python -m eqxvision_amd.build): per-block wall-clock stamps at
                       // prologue / main loop / epilogue boundaries, and for block 0 the shader-clock of every barrier exit
    long long pt0 = 0, pt1 = 0, pt2 = 0;
    int nstamp = 0;
    unsigned* stamps = (unsigned*)(smem + (LNF == 2 ? LDS_TOTAL_LN : LDS_TOTAL)) + wave * 128;
    if (p.prof) pt0 = wall_clock64();
#define MV_I8_STAMP()                                                                                      \
    do {                                                                                                   \
        if (p.prof && blockIdx.x == 0 && nstamp < 128) {                                                   \
            const unsigned tt = (unsigned)__builtin_readcyclecounter();                                    \
            if (lane == 0) stamps[nstamp] = tt;                                                            \
            ++nstamp;                                                                                      \
        }                                                                                                  \
    } while (0)
#else
#define MV_I8_STAMP() do {} while (0)
#endif
#ifdef MV_I8_PROF
    if (p.skew > 0 && blockIdx.x < 256) {          // experiment (i8_skew, debug build): de-phase the first round of workgroups by quarters
        const int q = (blockIdx.x >> 3) & 3;
        if (q) {
            const long long t_end = wall_clock64() + (long long)q * p.skew;
            while (wall_clock64() < t_end) __builtin_amdgcn_s_sleep(16);
        }
    }
#endif
    const int t = xcd_remap(blockIdx.x, p.tiles_m * p.tiles_n);
    int tile_m, tile_n;
    tile_coords(t, p.tiles_m, p.tiles_n, tile_m, tile_n, p.gm);
    const int m0 = tile_m * BM, n0 = tile_n * BN;

    // ---------------- DMA addressing ---------------------------------------------------------------------
    // One DMA instruction = 512 lanes x 16 bytes = 64 rows of 128 bytes; wave w stages rows 8 w .. 8 w + 7 of it.
    const int srow = lane >> 3;
    const int gch = (lane & 7) ^ ((4 * wave + (lane >> 4)) & 7);      // source chunk of LDS slot lane & 7 (swizzle)
    const int nk1 = p.R * p.S * (p.C >> 6);
    const int nk = DUAL ? nk1 + (p.C2 >> 6) : nk1;
    const unsigned wrow_bytes = 2u * (unsigned)(p.R * p.S * p.C + (DUAL ? p.C2 : 0));
    const RowBase rb = row_base(p, m0);
    const u32x4 rx = make_rsrc((const char*)p.x - rb.padb);
    const u32x4 rw = make_rsrc(p.w);
    u32x4 rx2 = rx;
    if constexpr (DUAL) rx2 = make_rsrc(p.x2);

    // x rows: slot q = 0 / 1 -> Xtop rows of group 0 / 1, q = 2 / 3 -> Xbot rows of group 0 / 1
    unsigned xvo[4], xmask[4];
    unsigned xvo2[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        xvo2[q] = OOB;
        row_setup<DUAL>(p, rb, m0, 128 * (q & 1) + 64 * (q >> 1) + 8 * wave + srow, gch, xvo[q], xmask[q], xvo2[q]);
    }
    unsigned wvo[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int n = n0 + 64 * j + 8 * wave + srow;
        wvo[j] = n < p.K ? (unsigned)n * wrow_bytes + 16u * (unsigned)gch : OOB;
    }
    const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) char*)smem;
    const unsigned ldsw = __builtin_amdgcn_readfirstlane(lds0 + wave * (8 * ROWB));

    auto tap_adv = [&](TapState& s, int tile) {
        if constexpr (DENSE) { s.woff += 128u; s.xoff += 128u; }     // the next 64 channels of both operands
        else tap_next<DUAL>(p, s, tile, nk1);
    };
    // the pieces of one k-tile: W x4, Xtop x2 (group 0 rows, group 1 rows), Xbot x2; BUF compile-time
    auto x_piece = [&](int q, const TapState& s, int tile, auto loff) {
        constexpr int LOFF = decltype(loff)::value;
        if (DUAL && tile >= nk1) {
            if constexpr (DUAL) dma16<LOFF>(ldsw, xvo2[q], rx2, s.xoff);
        } else if constexpr (DENSE) {
            dma16<LOFF>(ldsw, xvo[q], rx, s.xoff);        // rows past M carry OOB themselves; no taps
        } else {
            const unsigned vo = (xmask[q] & s.bit) ? xvo[q] : OOB;
            dma16<LOFF>(ldsw, vo, rx, s.xoff);
        }
    };
#define MV_I8_W(BUF, st)                                                           \
    do {                                                                           \
        dma16<LDS_W + (BUF) * 32768 + 0 * 8192>(ldsw, wvo[0], rw, (st).woff);      \
        dma16<LDS_W + (BUF) * 32768 + 1 * 8192>(ldsw, wvo[1], rw, (st).woff);      \
        dma16<LDS_W + (BUF) * 32768 + 2 * 8192>(ldsw, wvo[2], rw, (st).woff);      \
        dma16<LDS_W + (BUF) * 32768 + 3 * 8192>(ldsw, wvo[3], rw, (st).woff);      \
    } while (0)
#define MV_I8_X(BUF, q, st, tile)                                                                                     \
    x_piece(q, st, tile,                                                                                               \
            std::integral_constant<int, ((q) < 2 ? LDS_XT : LDS_XB) + (BUF) * 16384 + ((q) & 1) * 8192>{})

    // ---------------- fragment addressing ----------------------------------------------------------------
    const int fr = lane & 31, fh = lane >> 5, swz = (fr >> 1) & 7;
    unsigned waddr[4], xaddr[4];
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
        const unsigned ko = (unsigned)(((2 * kk + fh) ^ swz) << 4);
        waddr[kk] = lds0 + LDS_W + (64 * wc + fr) * ROWB + ko;
        xaddr[kk] = lds0 + LDS_XT + (64 * grp + fr) * ROWB + ko;
    }

    // ---------------- epilogue constants (older than every DMA: vmcnt retires in order) ------------------
#ifdef MV_I8_PROF
    const OutT* res = (p.dbg & 8) ? nullptr : (const OutT*)p.residual;       // ablation: no residual loads
    const bool do_store = !(p.dbg & 4);                                       // ablation: no global stores
#else
    const OutT* res = (const OutT*)p.residual;
    constexpr bool do_store = true;
#endif
    ScaleShift8 ss;
    if constexpr (LIN) ss.load_shift(p.shift, n0 + 64 * wc + (lane & 7) * 8, p.K);
    else ss.load(p.scale, p.shift, n0 + 64 * wc + (lane & 7) * 8, p.K);

    f32x16 acc[2][4];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[a][b][e] = 0.f;

    // ---------------- prologue: all of k-tile 0, and the phase-2 share (W, Xtop rows of group 0) of k-tile 1 ----
    TapState sa = tap_first();      // state of the tile whose W / Xtop(0) pieces are issued next (phase-2 issue)
    TapState sb = tap_first();      // state of the tile whose Xtop(1) / Xbot pieces are issued next (phase-1 issue)
    if constexpr (LNF == 2) {       // piece j of rows m0 .. m0 + 255 = 512 consecutive dwords of the table: one per thread
        const u32x4 rs = make_rsrc(p.stats_in);
        const unsigned ldsw4 = __builtin_amdgcn_readfirstlane(lds0 + wave * 256);
        const unsigned svo = m0 + (tid >> 1) < p.M ? 4u * (unsigned)(2 * m0 + tid) : OOB;
        const unsigned pstep = 8u * (unsigned)p.M;
        const int P = (p.C + 255) >> 8;
#define MV_I8_LNP(j) if ((j) < P) dma4<LDS_LNP + (j) * 2048>(ldsw4, svo, rs, (unsigned)(j) * pstep)
        MV_I8_LNP(0); MV_I8_LNP(1); MV_I8_LNP(2);
#undef MV_I8_LNP
    }
    MV_I8_W(0, sa);
    MV_I8_X(0, 0, sa, 0);
    MV_I8_X(0, 1, sb, 0);
    MV_I8_X(0, 2, sb, 0);
    MV_I8_X(0, 3, sb, 0);
    // LNF 2: the rows' (-mean * rstd, rstd) from the producers' pieces, while the first k-tile is still on its way (every wave's pieces
    // have landed once all waves are past their counted wait: one barrier); the epilogue reads the table many barriers later.
    auto ln_finalize = [&]() {
        __builtin_amdgcn_s_barrier();
        // Chan's merge of the P pieces (n_j = 256 values, the last one what is left of C): mean = sum(s_j) / C,
        // M2 = sum(q_j) + sum(n_j (s_j / n_j - mean)^2).  The reads are issued unconditionally and back to back (pieces >= P: whatever
        // the LDS holds, dropped by a select): guarded reads were dependent LDS round trips, 1.1 us per tile with twelve pieces.
        if (tid < 256) {
            const int P = (p.C + 255) >> 8;
            const unsigned a0 = lds0 + LDS_LNP + 8u * (unsigned)tid;
            u32x2 pc[LN_MAXP];
#define MV_I8_RD(j) asm volatile("ds_read_b64 %0, %1 offset:%2" : "=v"(pc[j]) : "v"(a0), "n"((j) * 2048) : "memory")
            MV_I8_RD(0); MV_I8_RD(1); MV_I8_RD(2);
#undef MV_I8_RD
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
            for (int j = 0; j < LN_MAXP; ++j) asm volatile("" : "+v"(pc[j]));
            float tot = 0.f;
#pragma unroll
            for (int j = 0; j < LN_MAXP; ++j) tot += j < P ? __uint_as_float(pc[j][0]) : 0.f;
            const float inv_n = 1.0f / (float)p.C, mean = tot * inv_n;
            float m2 = 0.f;
#pragma unroll
            for (int j = 0; j < LN_MAXP; ++j) {
                const float nj = (float)min(256, p.C - 256 * j);
                const float d = __uint_as_float(pc[j][0]) / nj - mean;
                m2 += j < P ? __uint_as_float(pc[j][1]) + nj * d * d : 0.f;
            }
            const float rstd = 1.0f / sqrtf(m2 * inv_n + p.ln_eps);
            *(float2*)(smem + LDS_LNS + 8 * tid) = make_float2(-mean * rstd, rstd);
        }
    };
    if (nk > 1) {
        tap_adv(sa, 1);
        MV_I8_W(1, sa);
        MV_I8_X(1, 0, sa, 1);
        if constexpr (LNF == 2) { wait_vm<13>(); ln_finalize(); }      // the statistics pieces are older than the 13 operand pieces
        wait_vm<7>();
    } else {
        if constexpr (LNF == 2) { wait_vm<8>(); ln_finalize(); }
        wait_vm<2>();
    }
    __builtin_amdgcn_s_barrier();
    if (grp == 1) __builtin_amdgcn_s_barrier();          // group 1 runs one barrier behind
#ifdef MV_I8_PROF
    if (p.prof) pt1 = wall_clock64();
#endif
    MV_I8_STAMP();

    u32x4 wf[2][4], xf[2][4];
    auto mfma_half = [&](int half) {
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int kk = 0; kk < 4; ++kk)
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int b = 0; b < 2; ++b)
                    acc[a][2 * half + b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                        __builtin_bit_cast(bf16x8, wf[a][kk]), __builtin_bit_cast(bf16x8, xf[b][kk]), acc[a][2 * half + b], 0, 0, 0);
        __builtin_amdgcn_s_setprio(0);
        __builtin_amdgcn_sched_barrier(0);
    };
    auto pin_frags = [&]() {        // every MFMA below depends on this point (the waits above it)
#pragma unroll
        for (int kk = 0; kk < 4; ++kk)
            asm volatile("" : "+v"(wf[0][kk]), "+v"(wf[1][kk]), "+v"(xf[0][kk]), "+v"(xf[1][kk]));
    };

    // one k-tile; BUF = it & 1 is a template value so that every LDS offset is an instruction immediate
    auto ktile = [&](int it, auto bufc) {
        constexpr int BUF = decltype(bufc)::value;
        // ---- phase 1 LOAD: weights + top pixel rows of tile `it`; issue Xtop(1) / Xbot of tile it+1 into the other buffer
#ifdef MV_I8_PROF
        const bool do_reads = !(p.dbg & 2), do_dma = !(p.dbg & 1);       // ablation (results wrong): what bounds an interval
#else
        constexpr bool do_reads = true, do_dma = true;
#endif
        if (do_reads) {
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                lds_read16<BUF * 32768>(wf[0][kk], waddr[kk]);
                lds_read16<BUF * 32768 + 32 * ROWB>(wf[1][kk], waddr[kk]);
            }
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                lds_read16<BUF * 16384>(xf[0][kk], xaddr[kk]);
                lds_read16<BUF * 16384 + 32 * ROWB>(xf[1][kk], xaddr[kk]);
            }
        }
        if (!do_dma) {
            wait_vm_lgkm0<0>();
        } else if (it + 1 < nk) {
            tap_adv(sb, it + 1);
            MV_I8_X(BUF ^ 1, 1, sb, it + 1);
            MV_I8_X(BUF ^ 1, 2, sb, it + 1);
            MV_I8_X(BUF ^ 1, 3, sb, it + 1);
            wait_vm_lgkm0<8>();          // Xbot of tile `it` (issued a k-tile ago) has landed
        } else {
            wait_vm_lgkm0<0>();
        }
        pin_frags();
        __builtin_amdgcn_s_barrier();
        MV_I8_STAMP();
        mfma_half(0);
        __builtin_amdgcn_s_barrier();
        MV_I8_STAMP();
        // ---- phase 2 LOAD: bottom pixel rows of tile `it`; issue W / Xtop(0) of tile it+2 into this buffer
        if (do_reads) {
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                lds_read16<(LDS_XB - LDS_XT) + BUF * 16384>(xf[0][kk], xaddr[kk]);
                lds_read16<(LDS_XB - LDS_XT) + BUF * 16384 + 32 * ROWB>(xf[1][kk], xaddr[kk]);
            }
        }
        if (!do_dma) {
            wait_vm_lgkm0<0>();
        } else if (it + 2 < nk) {
            tap_adv(sa, it + 2);
            MV_I8_W(BUF, sa);
            MV_I8_X(BUF, 0, sa, it + 2);
            wait_vm_lgkm0<7>();          // W and both Xtop pieces of tile it+1 have landed
        } else if (it + 1 < nk) {
            wait_vm_lgkm0<2>();
        } else {
            wait_vm_lgkm0<0>();
        }
        pin_frags();
        __builtin_amdgcn_s_barrier();
        MV_I8_STAMP();
        mfma_half(1);
        __builtin_amdgcn_s_barrier();
        MV_I8_STAMP();
    };
    for (int it = 0; it < nk; it += 2) {
        ktile(it, std::integral_constant<int, 0>{});
        if (it + 1 < nk) ktile(it + 1, std::integral_constant<int, 1>{});
    }
    if (grp == 0) __builtin_amdgcn_s_barrier();          // balance group 1's extra barrier: nobody reads LDS any more
#ifdef MV_I8_PROF
    if (p.prof) pt2 = wall_clock64();
#endif

    // ---------------- epilogue (igemm2's wave-private LDS transpose; branch-free buffer loads / stores: igemm_pipe.h) ----
    if constexpr (LNF == 0 || LNF == 2)
        epilogue_rows<OutT, LIN, 4, EPITCH, LNF>(p, smem + wave * (32 * EPITCH), acc, ss, res, do_store, m0 + 128 * grp, n0 + 64 * wc, lane,
                                                 smem + LDS_LNS + 1024 * grp);
    else
    {
        epilogue_rows_ln<LNF != 1, LNF != 4, 4, EPITCH>(p, smem + wave * (32 * EPITCH), acc, ss, do_store, m0 + 128 * grp, n0 + 64 * wc, lane,
                                                        smem + LDS_LN_SLOTS + 128 * 32 * grp, wc, smem + LDS_LN_DUMMY + 512 * wave);
        if constexpr (LNF != 4) {
            __syncthreads();
            if (tid < 256 && do_store) merge_row_stats(p, smem + LDS_LN_SLOTS, tid, m0, tile_n, min(4, (p.K - n0) >> 6));
        }
    }
#ifdef MV_I8_PROF
    if (p.prof) {
        if (tid == 0) {
            long long* o = p.prof + 4ll * blockIdx.x;
            o[0] = pt0; o[1] = pt1; o[2] = pt2; o[3] = wall_clock64();
        }
        if (blockIdx.x == 0 && lane == 0) {               // barrier stamps of the 8 waves behind the per-block table
            long long* o = p.prof + 4ll * gridDim.x + wave * 128;
            for (int i = 0; i < 128; ++i) o[i] = i < nstamp ? (long long)stamps[i] : -1;
        }
    }
#endif
#undef MV_I8_STAMP
#undef MV_I8_W
#undef MV_I8_X
}

// ---------------------------------------------------------------------------------------------------------------------
// The same ping-pong for layers with too few 256 x 256 tiles: a wave owns 64 x 64 (4 MFMA tiles, 64 accumulator registers),
// a k-tile of 64 is ONE phase (LOAD: 16 ds_read_b128 + the thread's 6 DMA pieces of the tile two ahead; MFMA: 16 MFMAs),
// LDS is a ring of three 48 KB k-tiles (`vmcnt(6)`: one whole tile in flight across the barriers).
//   ARR = 0: block = 128 pixels x 256 channels (group g: pixel rows 64 g ..; its four waves: 64 channels each) -- layers
//            with few pixel rows (ResNet 14 x 14 / 7 x 7 maps at half batch, Swin stages 2-3);
//   ARR = 1: block = 256 pixels x 128 channels (group g: pixel rows 128 g ..; its waves 2 (pixels) x 2 (channels)) -- layers
//            with 128 output channels (ResNet layer2).
// Per FLOP it stages 1.5x the bytes of the 256 x 256 tile, so it is the slower kernel wherever both fill the chip.
template <typename OutT, int ARR, bool DUAL, bool DENSE = false>
__global__ __launch_bounds__(512) void igemm8s_kernel(const Igemm2P p) {
    static_assert(!(DUAL && DENSE), "DENSE is single-source");
    constexpr int BM = ARR == 0 ? 128 : 256, BN = ARR == 0 ? 256 : 128;
    constexpr int ROWB = 128;
    constexpr int XI = BM / 64, WI = BN / 64;              // DMA pieces per thread per k-tile
    constexpr int XBYTES = BM * ROWB;                       // the x unit comes first in a ring slot, then the w unit
    constexpr int SLOT = (BM + BN) * ROWB;                  // 48 KB
    constexpr int EPITCH = 64 * 4 + 16;
    static_assert(XI + WI == 6 && 3 * SLOT <= 160 * 1024 && 8 * 32 * EPITCH <= 3 * SLOT, "ring layout");
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int grp = wave >> 2;
    const int xrow0 = ARR == 0 ? 64 * grp : 128 * grp + 64 * (wave & 1);
    const int wrow0 = ARR == 0 ? 64 * (wave & 3) : 64 * ((wave >> 1) & 1);
    // split-K (p.sync != nullptr): the two halves of a tile's reduction are blocks b and b + 8 -- dispatched together, on the
    // same XCD (one L2 between the partial sums' writer and reader)
    const bool splitk = p.sync != nullptr;
    int t = blockIdx.x, half = 0;
    if (splitk) {
        t = (blockIdx.x >> 4) * 8 + (blockIdx.x & 7);
        half = (blockIdx.x >> 3) & 1;
        if (t >= p.tiles_m * p.tiles_n) return;
    }
    t = xcd_remap(t, p.tiles_m * p.tiles_n);
    int tile_m, tile_n;
    tile_coords(t, p.tiles_m, p.tiles_n, tile_m, tile_n, p.gm);
    const int m0 = tile_m * BM, n0 = tile_n * BN;

    const int srow = lane >> 3;
    const int gch = (lane & 7) ^ ((4 * wave + (lane >> 4)) & 7);
    const int nk1 = p.R * p.S * (p.C >> 6);
    const int nk_all = DUAL ? nk1 + (p.C2 >> 6) : nk1;
    const int k0 = half ? (nk_all + 1) >> 1 : 0;                      // this block's k-tiles: k0 .. k0 + nk - 1
    const int nk = splitk ? (half ? nk_all - k0 : (nk_all + 1) >> 1) : nk_all;
    const unsigned wrow_bytes = 2u * (unsigned)(p.R * p.S * p.C + (DUAL ? p.C2 : 0));
    const RowBase rb = row_base(p, m0);
    const u32x4 rx = make_rsrc((const char*)p.x - rb.padb);
    const u32x4 rw = make_rsrc(p.w);
    u32x4 rx2 = rx;
    if constexpr (DUAL) rx2 = make_rsrc(p.x2);
    unsigned xvo[XI], xmask[XI], xvo2[XI];
#pragma unroll
    for (int q = 0; q < XI; ++q) {
        xvo2[q] = OOB;
        row_setup<DUAL>(p, rb, m0, 64 * q + 8 * wave + srow, gch, xvo[q], xmask[q], xvo2[q]);
    }
    unsigned wvo[WI];
#pragma unroll
    for (int j = 0; j < WI; ++j) {
        const int n = n0 + 64 * j + 8 * wave + srow;
        wvo[j] = n < p.K ? (unsigned)n * wrow_bytes + 16u * (unsigned)gch : OOB;
    }
    const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) char*)smem;
    const unsigned ldsw = __builtin_amdgcn_readfirstlane(lds0 + wave * (8 * ROWB));

    auto tap_adv = [&](TapState& s, int tile) {
        if constexpr (DENSE) { s.woff += 128u; s.xoff += 128u; }
        else tap_next<DUAL>(p, s, tile, nk1);
    };
    auto stage = [&](const TapState& st, int tile, auto slotc) {
        constexpr int BASE = decltype(slotc)::value * SLOT;
        const bool second = DUAL && tile >= nk1;
        if (second) {
            if constexpr (DUAL) {
                dma16<BASE + 0 * 8192>(ldsw, xvo2[0], rx2, st.xoff);
                dma16<BASE + 1 * 8192>(ldsw, xvo2[1], rx2, st.xoff);
                if constexpr (XI == 4) {
                    dma16<BASE + 2 * 8192>(ldsw, xvo2[2], rx2, st.xoff);
                    dma16<BASE + 3 * 8192>(ldsw, xvo2[3], rx2, st.xoff);
                }
            }
        } else if constexpr (DENSE) {
            dma16<BASE + 0 * 8192>(ldsw, xvo[0], rx, st.xoff);
            dma16<BASE + 1 * 8192>(ldsw, xvo[1], rx, st.xoff);
            if constexpr (XI == 4) {
                dma16<BASE + 2 * 8192>(ldsw, xvo[2], rx, st.xoff);
                dma16<BASE + 3 * 8192>(ldsw, xvo[3], rx, st.xoff);
            }
        } else {
            dma16<BASE + 0 * 8192>(ldsw, (xmask[0] & st.bit) ? xvo[0] : OOB, rx, st.xoff);
            dma16<BASE + 1 * 8192>(ldsw, (xmask[1] & st.bit) ? xvo[1] : OOB, rx, st.xoff);
            if constexpr (XI == 4) {
                dma16<BASE + 2 * 8192>(ldsw, (xmask[2] & st.bit) ? xvo[2] : OOB, rx, st.xoff);
                dma16<BASE + 3 * 8192>(ldsw, (xmask[3] & st.bit) ? xvo[3] : OOB, rx, st.xoff);
            }
        }
        dma16<BASE + XBYTES + 0 * 8192>(ldsw, wvo[0], rw, st.woff);
        dma16<BASE + XBYTES + 1 * 8192>(ldsw, wvo[1], rw, st.woff);
        if constexpr (WI == 4) {
            dma16<BASE + XBYTES + 2 * 8192>(ldsw, wvo[2], rw, st.woff);
            dma16<BASE + XBYTES + 3 * 8192>(ldsw, wvo[3], rw, st.woff);
        }
    };

    // fragment addresses: set A reaches ring slots 0 and 1 through the instruction offset, set B is slot 2
    const int fr = lane & 31, fh = lane >> 5, swz = (fr >> 1) & 7;
    unsigned waddr[4], xaddr[4], waddr2[4], xaddr2[4];
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
        const unsigned ko = (unsigned)(((2 * kk + fh) ^ swz) << 4);
        xaddr[kk] = lds0 + (xrow0 + fr) * ROWB + ko;
        waddr[kk] = lds0 + XBYTES + (wrow0 + fr) * ROWB + ko;
        xaddr2[kk] = xaddr[kk] + 2 * SLOT;
        waddr2[kk] = waddr[kk] + 2 * SLOT;
    }

    const OutT* res = (const OutT*)p.residual;
    ScaleShift8 ss;
    ss.load(p.scale, p.shift, n0 + wrow0 + (lane & 7) * 8, p.K);

    f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[a][b][e] = 0.f;

    TapState st = tap_first();
    if (k0) {
        if constexpr (DENSE) { st.woff = st.xoff = 128u * (unsigned)k0; }
        else st = tap_at<DUAL>(p, k0, nk1);
    }
    stage(st, k0, std::integral_constant<int, 0>{});
    if (nk > 1) {
        tap_adv(st, k0 + 1);
        stage(st, k0 + 1, std::integral_constant<int, 1>{});
        wait_vm<6>();
    } else {
        wait_vm<0>();
    }
    __builtin_amdgcn_s_barrier();
    if (grp == 1) __builtin_amdgcn_s_barrier();          // group 1 runs one barrier behind

    u32x4 wf[2][4], xf[2][4];
    auto ktile = [&](int it, auto slotc) {
        constexpr int SL = decltype(slotc)::value;          // ring slot of tile `it` (it counts from this block's first k-tile)
        constexpr int OFF = SL == 2 ? 0 : SL * SLOT;
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            lds_read16<OFF>(wf[0][kk], SL == 2 ? waddr2[kk] : waddr[kk]);
            lds_read16<OFF + 32 * ROWB>(wf[1][kk], SL == 2 ? waddr2[kk] : waddr[kk]);
            lds_read16<OFF>(xf[0][kk], SL == 2 ? xaddr2[kk] : xaddr[kk]);
            lds_read16<OFF + 32 * ROWB>(xf[1][kk], SL == 2 ? xaddr2[kk] : xaddr[kk]);
        }
        if (it + 2 < nk) {                                   // tile it+2 goes where tile it-1 was (last read a phase ago)
            tap_adv(st, k0 + it + 2);
            stage(st, k0 + it + 2, std::integral_constant<int, (SL + 2) % 3>{});
            wait_vm_lgkm0<6>();                              // tile it+1 has landed
        } else {
            wait_vm_lgkm0<0>();
        }
#pragma unroll
        for (int kk = 0; kk < 4; ++kk)
            asm volatile("" : "+v"(wf[0][kk]), "+v"(wf[1][kk]), "+v"(xf[0][kk]), "+v"(xf[1][kk]));
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int kk = 0; kk < 4; ++kk)
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int b = 0; b < 2; ++b)
                    acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, wf[a][kk]),
                                                                        __builtin_bit_cast(bf16x8, xf[b][kk]), acc[a][b], 0, 0, 0);
        __builtin_amdgcn_s_setprio(0);
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();
    };
    for (int it = 0; it < nk; it += 3) {
        ktile(it, std::integral_constant<int, 0>{});
        if (it + 1 < nk) ktile(it + 1, std::integral_constant<int, 1>{});
        if (it + 2 < nk) ktile(it + 2, std::integral_constant<int, 2>{});
    }
    if (grp == 0) __builtin_amdgcn_s_barrier();

    if (splitk) {
        // Two-way split-K, deterministic: whichever half of a tile finishes FIRST parks its fp32 accumulators (in register order,
        // 16 bytes per lane: coalesced) and leaves; the other half adds them to its own -- a + b == b + a bit for bit, so the
        // result does not depend on which one that was -- and runs the epilogue.  The second block only ever waits for a block
        // that is already past its main loop (no dependence on dispatch order), and it leaves both words zero for the next launch.
        // Visibility: the two blocks normally sit on one XCD (one L2; a CU's vector L1 is write-through and cannot hold a line of
        // the partial tile, which nobody has read in this launch), so the hand-over needs no cache maintenance; the writer still
        // publishes with ONE release (a single L2 write-back, not one per wave) and says which XCD it ran on, and a reader on a
        // different XCD -- not seen with today's round-robin dispatch, but nothing promises it -- invalidates before it reads.
        unsigned* sync = p.sync + 2 * t;
        float4* part = (float4*)p.ws + (size_t)t * (BM * BN / 4) + tid;
        const unsigned xcc = __builtin_amdgcn_s_getreg(20 | (3 << 11)) & 15u;                 // HW_REG_XCC_ID[3:0]
        if (tid == 0) *(volatile unsigned*)smem = __hip_atomic_fetch_add(sync, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __syncthreads();
        const unsigned arrived = *(volatile unsigned*)smem;
        __syncthreads();
        if (arrived == 0) {
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int b = 0; b < 2; ++b)
#pragma unroll
                    for (int g = 0; g < 4; ++g)
                        part[((a * 2 + b) * 4 + g) * 512] = make_float4(acc[a][b][4 * g + 0], acc[a][b][4 * g + 1],
                                                                        acc[a][b][4 * g + 2], acc[a][b][4 * g + 3]);
            __syncthreads();                                 // every wave's stores have reached the L2 (s_waitcnt vmcnt(0) + barrier)
            if (tid == 0) __hip_atomic_store(sync + 1, 1u + xcc, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
            return;
        }
        if (tid == 0) {
            int spins = 0;                                   // bounded (~0.1 s): never a hung GPU -- and never a SILENTLY wrong tile:
            unsigned f;                                      // the partner is past its main loop when this block gets here, so running
            while ((f = __hip_atomic_load(sync + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) == 0u && ++spins < (1 << 20))
                __builtin_amdgcn_s_sleep(2);                 // out of spins means a broken hand-over (dirty sync words, or a partner that
            if (f == 0u)                                     // was never co-resident): say so in the status word -- the host checks it
                __hip_atomic_fetch_or(&g_dev_status, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // (mv_device_status) -- and go on
            if (f != 1u + xcc) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            __hip_atomic_store(sync, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(sync + 1, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        __syncthreads();
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const float4 o = part[((a * 2 + b) * 4 + g) * 512];
                    acc[a][b][4 * g + 0] += o.x; acc[a][b][4 * g + 1] += o.y; acc[a][b][4 * g + 2] += o.z; acc[a][b][4 * g + 3] += o.w;
                }
    }

    epilogue_rows<OutT, false, 2, EPITCH>(p, smem + wave * (32 * EPITCH), acc, ss, res, true, m0 + xrow0, n0 + wrow0, lane);
}

// -> the status word (and clears it when asked).  Synchronises the device: call it where the host synchronises anyway.
int device_status(int clear, unsigned* out) {
    unsigned v = 0;
    MV_HIP(hipMemcpyFromSymbol(&v, HIP_SYMBOL(g_dev_status), sizeof(v), 0, hipMemcpyDeviceToHost));
    if (clear && v) {
        const unsigned z = 0;
        MV_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_dev_status), &z, sizeof(z), 0, hipMemcpyHostToDevice));
    }
    *out = v;
    return MV_OK;
}

// the word's address on the current device, for kernels of other translation units (a __device__ variable is private to its own)
unsigned* device_status_word() {
    void* p = nullptr;
    if (hipGetSymbolAddress(&p, HIP_SYMBOL(g_dev_status)) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    return (unsigned*)p;
}

size_t splitk_scratch_bytes(long long M, long long N, long long kred) {
    if (N <= 0 || M <= 0) return 0;
    // which of the two half-size shapes the dispatch picks is its business: room for the one with more tiles
    const long long ta = ((M + 127) / 128) * ((N + 255) / 256), tb = ((M + 255) / 256) * ((N + 127) / 128);
    if (!splitk_rule(ta < tb ? ta : tb, kred / 64, get_flag)) return 0;
    return SPLITK_SYNC_BYTES + (size_t)(ta > tb ? ta : tb) * 128 * 256 * 4;
}

static int igemm8_go(Igemm2P& p, bool dual, bool out_f32, int tile, hipStream_t st) {
    const int bm = tile == 1 ? 128 : 256, bn = tile == 2 ? 128 : 256;
    p.tiles_m = (p.M + bm - 1) / bm;
    p.tiles_n = (p.K + bn - 1) / bn;
    p.gm = 8;             // 1 ... 12 are equal on the ViT shapes, 32+ lose 7 % (profiles/r05/vit_tile_order_gm_sweep.txt)
#ifdef MV_I8_PROF
    p.skew = get_flag("i8_skew");                    // measured -3.6 % on vit_base (profiles/r04/vit_ab_i8_skew_4.6us.txt)
#endif
    const int tiles = p.tiles_m * p.tiles_n;
    p.sync = nullptr; p.ws = nullptr;
    const size_t need = tile != 0 ? splitk_need_bytes(tiles, (long long)p.R * p.S * (p.C / 64) + (dual ? p.C2 / 64 : 0), get_flag) : 0;
    if (need) {
        void* sc = take_scratch(st, need);                               // the host's mv_set_scratch for this launch
        if (sc) { p.sync = (unsigned*)sc; p.ws = (float*)((char*)sc + SPLITK_SYNC_BYTES); }
    }
    const dim3 grid((unsigned)(p.sync ? 16 * ((tiles + 7) / 8) : tiles)), block(512);
#define GO(KERN, SMEM)                                                                                            \
    do {                                                                                                          \
        auto kern = KERN;                                                                                         \
        static LdsAttrSite attr;                                                                                  \
        MV_HIP(attr.ensure((const void*)kern, SMEM));                                                             \
        hipLaunchKernelGGL(kern, grid, block, SMEM, st, p);                                                       \
    } while (0)
#define GO4(NAME, SMEM, ...)                                                  \
    do {                                                                      \
        if (dual) {                                                           \
            if (out_f32) GO((NAME<float, ##__VA_ARGS__, true>), SMEM);        \
            else GO((NAME<bf16_t, ##__VA_ARGS__, true>), SMEM);               \
        } else {                                                              \
            if (out_f32) GO((NAME<float, ##__VA_ARGS__, false>), SMEM);       \
            else GO((NAME<bf16_t, ##__VA_ARGS__, false>), SMEM);              \
        }                                                                     \
    } while (0)
    const bool dense1 = !dual && p.R == 1 && p.S == 1 && p.sh == 1 && p.sw == 1 && p.ph == 0 && p.pw == 0 && !get_flag("no_i8_lin");
#ifdef MV_I8_PROF
    constexpr int PROF_PAD = 4096;
#else
    constexpr int PROF_PAD = 0;
#endif
    if (p.stats_out && !p.residual2) GO((igemm8_kernel<float, false, 2, 1>), LDS_TOTAL + PROF_PAD);   // igemm8_ln*_launch: tile 0, dense, checked there
    else if (p.stats_out) GO((igemm8_kernel<float, false, 2, 3>), LDS_TOTAL + PROF_PAD);
    else if (p.residual2) GO((igemm8_kernel<float, false, 2, 4>), LDS_TOTAL + PROF_PAD);
    else if (p.stats_in) GO((igemm8_kernel<bf16_t, false, 1, 2>), LDS_TOTAL_LN + PROF_PAD);
    else if (tile == 1 && dense1) {
        if (out_f32) GO((igemm8s_kernel<float, 0, false, true>), 3 * 384 * 128);
        else GO((igemm8s_kernel<bf16_t, 0, false, true>), 3 * 384 * 128);
    } else if (tile == 2 && dense1) {
        if (out_f32) GO((igemm8s_kernel<float, 1, false, true>), 3 * 384 * 128);
        else GO((igemm8s_kernel<bf16_t, 1, false, true>), 3 * 384 * 128);
    } else if (tile == 1) GO4(igemm8s_kernel, 3 * 384 * 128, 0);
    else if (tile == 2) GO4(igemm8s_kernel, 3 * 384 * 128, 1);
#ifdef MV_I8_PROF
    else GO4(igemm8_kernel, LDS_TOTAL + 4096);
#else
    else if (!dual && p.R == 1 && p.S == 1 && p.sh == 1 && p.sw == 1 && p.ph == 0 && p.pw == 0 && !get_flag("no_i8_lin")) {
        if (p.scale) {
            if (out_f32) GO((igemm8_kernel<float, false, 1>), LDS_TOTAL);
            else GO((igemm8_kernel<bf16_t, false, 1>), LDS_TOTAL);
        } else {
            if (out_f32) GO((igemm8_kernel<float, false, 2>), LDS_TOTAL);
            else GO((igemm8_kernel<bf16_t, false, 2>), LDS_TOTAL);
        }
    } else GO4(igemm8_kernel, LDS_TOTAL);
#endif
#undef GO4
#undef GO
    MV_LAUNCH_CHECK();
    return MV_OK;
}

int igemm8_launch(const void* x, const void* w, const float* scale, const float* shift, const void* residual, void* y,
                  const ConvShape& s, int tok, int tile, hipStream_t st) {
    Igemm2P p;
    memset(&p, 0, sizeof(p));
    p.tok = tok;
    p.x = (const bf16_t*)x; p.w = (const bf16_t*)w; p.scale = scale; p.shift = shift; p.residual = residual; p.y = y;
    p.N = s.N; p.H = s.H; p.W = s.W; p.C = s.C; p.K = s.K; p.R = s.R; p.S = s.S;
    p.Ho = s.Ho(); p.Wo = s.Wo();
    p.sh = s.sh; p.sw = s.sw; p.ph = s.ph; p.pw = s.pw; p.dh = s.dh; p.dw = s.dw;
    p.s2 = 1;
    const long long M = s.M();
    if (!igemm8_supported(M, s.C, s.K, s.R, s.S, 2LL * s.N * s.H * s.W * s.C, 2LL * s.K * s.R * s.S * s.C)) {
        set_error("igemm8: unsupported shape M=%lld C=%d K=%d R=%d S=%d", M, s.C, s.K, s.R, s.S);
        return MV_E_UNSUPPORTED;
    }
    p.M = (int)M;
    p.act = s.act;
#ifdef MV_I8_PROF
    p.prof = (long long*)(((unsigned long long)(unsigned)get_flag("prof_hi") << 32) | (unsigned)get_flag("prof_lo"));
    p.dbg = get_flag("i8_ablate");
#endif
    const int out_dtype = s.out_dtype;
    const int rc = igemm8_go(p, false, out_dtype == MV_F32, tile - 1, st);
    if (p.sync) append_kernel_name(kSplitkSuffix);
    return rc;
}

// The LayerNorm between two Linears folded into their epilogues (256 x 256 tiles; igemm_pipe.h: epilogue_rows_ln / epilogue_rows LNF 2).
//   producer: y[M][N] = residual + x[M][K] . w[N][K]^T + shift.  residual: fp32 rows (res_lo == nullptr) or two bf16 planes (res, res_lo);
//             y: two bf16 planes (y, y_lo) + stats[ceil(N / 256)][M][2], or fp32 rows (y_lo == stats == nullptr; needs res_lo)
//   consumer: y[M][N] bf16 (or head-major, tok > 0) = act(rstd[m] * (x[M][K] . w'[N][K]^T - mean[m] * colsum[n]) + shift'[n]),
//             x = the producer's high plane, (mean, rstd)[m] from its stats[ceil(K / 256)][M][2]
static bool igemm8_ln_supported(long long M, int N, int K) {
    return M >= 256 && M < (1LL << 24) && N % 64 == 0 && N >= 256 && K % 64 == 0 && K >= 256 &&
           igemm8_supported(M, K, N, 1, 1, 2LL * M * K, 2LL * N * K);
}

static void ln_params(Igemm2P& p, const void* x, const void* w, const float* shift, void* y, long long M, int N, int K) {
    memset(&p, 0, sizeof(p));
    p.x = (const bf16_t*)x; p.w = (const bf16_t*)w; p.shift = shift; p.y = y;
    p.N = 1; p.H = (int)M; p.W = 1; p.C = K; p.K = N; p.R = 1; p.S = 1; p.Ho = (int)M; p.Wo = 1;
    p.sh = 1; p.sw = 1; p.dh = 1; p.dw = 1; p.s2 = 1;
    p.M = (int)M;
}

static int igemm8_lnout_launch(const void* x, const void* w, const float* shift, const void* res, const void* res_lo, void* y,
                               void* y_lo, float* stats, long long M, int N, int K, hipStream_t st) {
    if (!igemm8_ln_supported(M, N, K) || !res || (!y_lo) != (!stats) || (!y_lo && !res_lo)) {
        set_error("igemm8 lnout: unsupported shape M=%lld N=%d K=%d or stream form", M, N, K);
        return MV_E_UNSUPPORTED;
    }
    Igemm2P p;
    ln_params(p, x, w, shift, y, M, N, K);
    p.residual = res; p.residual2 = res_lo; p.y2 = y_lo; p.stats_out = stats;
    set_kernel_name(!res_lo ? "igemm8_bf16_256x256_lin_lnout_f32res" : (y_lo ? "igemm8_bf16_256x256_lin_lnout" : "igemm8_bf16_256x256_lin_f32out_splitres"));
    return igemm8_go(p, false, true, 0, st);
}

static int igemm8_lnin_launch(const void* x, const float* stats, const void* w, const float* colsum, const float* shift, void* y,
                              long long M, int N, int K, float eps, int act, int tok, hipStream_t st) {
    if (!igemm8_ln_supported(M, N, K) || K > 256 * LN_MAXP) {
        set_error("igemm8 lnin: unsupported shape M=%lld N=%d K=%d", M, N, K);
        return MV_E_UNSUPPORTED;
    }
    Igemm2P p;
    ln_params(p, x, w, shift, y, M, N, K);
    p.scale = colsum; p.stats_in = stats; p.ln_eps = eps; p.act = act; p.tok = tok;
    set_kernel_name("igemm8_bf16_256x256_dense_lnin");
    return igemm8_go(p, false, false, 0, st);
}

// y[N,Ho,Wo,K] = act(scale[k] * (x[N,Ho,Wo,C1] . w[k, 0:C1] + x2[N, s2*ho, s2*wo, C2] . w[k, C1:C1+C2]) + shift[k] + residual)
int igemm8_dual_launch(const void* x, const void* x2, const void* w, const float* scale, const float* shift,
                       const void* residual, void* y, int N, int Ho, int Wo, int C1, int H2, int W2, int C2, int s2, int K,
                       int act, int out_dtype, int tile, hipStream_t st) {
    Igemm2P p;
    memset(&p, 0, sizeof(p));
    p.x = (const bf16_t*)x; p.w = (const bf16_t*)w; p.scale = scale; p.shift = shift; p.residual = residual; p.y = y;
    p.x2 = (const bf16_t*)x2; p.C2 = C2; p.H2 = H2; p.W2 = W2; p.s2 = s2;
    p.N = N; p.H = Ho; p.W = Wo; p.C = C1; p.K = K; p.R = 1; p.S = 1;
    p.Ho = Ho; p.Wo = Wo;
    p.sh = 1; p.sw = 1; p.ph = 0; p.pw = 0; p.dh = 1; p.dw = 1;
    const long long M = (long long)N * Ho * Wo;
    if (!igemm8_supported(M, C1, K, 1, 1, 2LL * M * C1, 2LL * K * (C1 + C2)) || C2 % 64 || C2 < 64 ||
        2LL * N * H2 * W2 * C2 >= (1LL << 31) - (1 << 22)) {
        set_error("igemm8 dual: unsupported shape M=%lld C1=%d C2=%d K=%d", M, C1, C2, K);
        return MV_E_UNSUPPORTED;
    }
    p.M = (int)M;
    p.act = act;
    const int rc = igemm8_go(p, true, out_dtype == MV_F32, tile - 1, st);
    if (p.sync) append_kernel_name(kSplitkSuffix);
    return rc;
}

}  // namespace mv

using namespace mv;

extern "C" {

// ---- the LayerNorm between two Linears folded into their epilogues (ViT: norm1 -> qkv, norm2 -> fc1) ----
// The pair is only worth it on the 256 x 256 tiles both GEMMs would take anyway (igemm8_wanted == 1 for BOTH shapes is the
// caller's business: ask _supported for each Linear of the pair).
int mv_linear_lnout_supported(int64_t M, int N, int K, int dtype) {
    return dtype == MV_BF16 && !get_flag("force_generic") && !get_flag("no_igemm8") && !get_flag("no_ln_fold") && igemm8_ln_supported(M, N, K) &&
           igemm8_wanted(M, K, N, 1, 1, get_flag) == 1;
}

int mv_linear_lnout_fwd(const void* x, const void* w, const float* shift, const void* res, const void* res_lo, void* y, void* y_lo,
                        float* stats, int64_t M, int N, int K, int dtype, mv_stream_t stream) {
    MV_CHECK_ARG(x && w && res && y, "linear_lnout: NULL pointer");
    MV_CHECK_ARG((y_lo != nullptr) == (stats != nullptr), "linear_lnout: y_lo and stats go together (planes out) or are both NULL (fp32 rows out)");
    MV_CHECK_ARG(y_lo || res_lo, "linear_lnout: fp32 rows in and out is mv_linear_fwd");
    MV_CHECK_ARG(y != x && y_lo != x, "linear_lnout: an output aliases the operand rows");
    if (!mv_linear_lnout_supported(M, N, K, dtype)) {
        set_error("linear_lnout: unsupported shape M=%lld N=%d K=%d (ask mv_linear_lnout_supported first)", (long long)M, N, K);
        return MV_E_UNSUPPORTED;
    }
    return igemm8_lnout_launch(x, w, shift, res, res_lo, y, y_lo, stats, M, N, K, (hipStream_t)stream);
}

int mv_linear_lnin_supported(int64_t M, int N, int K, int tokens, int dh, int dtype) {
    if (tokens > 0 && !(dh == 64 && M % tokens == 0 && mha_mfma_supported(tokens, dh, dtype))) return 0;
    return dtype == MV_BF16 && !get_flag("force_generic") && !get_flag("no_igemm8") && !get_flag("no_ln_fold") && K <= 768 &&
           igemm8_ln_supported(M, N, K) && igemm8_wanted(M, K, N, 1, 1, get_flag) == 1;
}

int mv_linear_lnin_fwd(const void* x, const float* stats, const void* w_folded, const float* colsum, const float* shift, void* y,
                       int64_t M, int N, int K, float eps, int act, int tokens, int dh, int dtype, mv_stream_t stream) {
    MV_CHECK_FUSED_ACT(act, "linear_lnin");
    MV_CHECK_ARG(x && stats && w_folded && colsum && y, "linear_lnin: NULL pointer");
    MV_CHECK_ARG(eps > 0.f, "linear_lnin: eps %g", (double)eps);
    if (!mv_linear_lnin_supported(M, N, K, tokens, dh, dtype)) {
        set_error("linear_lnin: unsupported shape M=%lld N=%d K=%d tokens=%d dh=%d (ask mv_linear_lnin_supported first)", (long long)M, N,
                  K, tokens, dh);
        return MV_E_UNSUPPORTED;
    }
    return igemm8_lnin_launch(x, stats, w_folded, colsum, shift, y, M, N, K, eps, act, tokens, (hipStream_t)stream);
}

}  // extern "C"
