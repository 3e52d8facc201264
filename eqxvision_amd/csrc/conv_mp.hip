// Mixed-precision Conv2d (groups == 1) for the training step: forward, input gradient and weight gradient as implicit GEMMs with bf16
// operands and fp32 accumulation on v_mfma_f32_32x32x16_bf16.  Maps are NHWC fp32, filters KRSC fp32, every tensor stays fp32 in
// memory; every operand element is rounded to bf16 (round-to-nearest-even) on its way into LDS, the result is stored as fp32.  No
// im2col buffer exists anywhere: a tile row of the gathered operand is looked up per tap when it is loaded.
//
//   entry   output tile rows x columns    gathered operand (rows)              plain operand                reduction, walked as
//   fwd     positions p x filters k       x  [in(p,r,s)][c]  contiguous        w [k][(r,s,c)] contiguous    (tap, 32 channels c)
//   dgrad   input positions q x chan. c   dy [out(q,r,s)][k] contiguous        w [k][(r,s) c] along rows    (tap, 32 filters k)
//   wgrad   filters k x channels c, 1 tap x  [in(p,r,s)][c]  along rows        dy [p][k]      along rows    32 positions p
// in(p, r, s)  = (n, ho sh - ph + r dh, wo sw - pw + s dw); outside the map it is padding: the row reads as zeros (BUF_OOB).
// out(q, r, s) = (n, (hi + ph - r dh) / sh, (wi + pw - s dw) / sw) where both divisions leave no remainder and the quotients lie in
// the output map; every other tap contributes nothing to that position ("the stride divides").
// A step never straddles two taps; channels / filters past the end of the last chunk of a tap read as zeros.
//
// Tile, LDS images, fragment reads, the MFMA step, the double-buffered loop (lmp_reduce), the store of a tile (lmp_store_tile) and the
// weight gradient's split rule (lmp_wgrad_split) are linear_mp.hip's, all in linear_mp_tile.h: 128 x 128 outputs per workgroup of 4 waves,
// 32 reduction elements per step, the next step's loads in registers, one barrier per step.  Here: the tile decoding, the walk over
// (tap, chunk), the loaders and the output base.  The plain operand is loaded with lmp_gload as it is; only the gathered operand has
// loaders of its own (cmp_gload_rows / cmp_gload_red), which produce the same register patch, so lmp_lstore / lmp_frag serve both.
// Deviations from linear_mp.hip, and why:
//   * wgrad's grid is (filter tiles x taps x channel tiles): the source row of a position depends on the tap, so a tile holds one tap.
//     With C = 3 (the stems) 125 of a tile's 128 columns are padding; the entry is correct there, not fast.
//   * dgrad walks every tap for every tile, also under a stride, where a position takes only 1 / (sh sw) of them: the rows of a tile
//     have mixed parities, so no tap can be skipped for the whole tile.
//   * the gathered operand has ONE buffer descriptor at the tensor's base (a tile's rows cross image boundaries), so the gathered map is
//     limited to 2^31 bytes; the entries refuse a larger one.  The plain operand is re-based per tile / per step as in linear_mp.hip.
//
// Resources (hipcc -O3 --offload-arch=gfx950, -Rpass-analysis=kernel-resource-usage; 256 threads, LDS 40960 bytes each; no spills, no scratch):
//   conv_mp_fwd_bf16             (cmp_kernel<0>)   VGPR  90  AGPR 64   3 waves / SIMD
//   conv_mp_dgrad_bf16           (cmp_kernel<1>)   VGPR 108  AGPR 64   2 waves / SIMD
//   conv_mp_wgrad[_split]_bf16   (cmp_kernel<2>)   VGPR  98  AGPR 64   3 waves / SIMD
// (the 64 accumulator registers live in AGPRs; LDS allows 3 workgroups of 4 waves per CU, i.e. 3 waves per SIMD.  For comparison,
// linear_mp.hip's lmp_kernel: fwd 80, dgrad 98 -- 3 waves / SIMD --, wgrad 112 VGPRs -- 2 waves / SIMD --, 64 AGPRs each.)
// The loader is a lambda lmp_reduce calls once per step: it keeps (tap, chunk) and the step in its own counters -- taking the step from
// the loop instead costs wgrad 8 VGPRs and its third wave.
#include "linear_mp_tile.h"

namespace mv {
namespace {

enum { CMP_FWD = 0, CMP_DGRAD = 1, CMP_WGRAD = 2 };

struct CmpP {
    const float* a;          // the gathered map: x (fwd, wgrad) or dy (dgrad)
    const float* b;          // the plain operand: w (fwd, dgrad) or dy (wgrad)
    const float* bias;       // [K] or null, added in fp32 (fwd)
    float* c;                // y / dx / dw, or the parts [gridDim.y][K R S C] of a split wgrad
    int H, W, C, K, R, S, sh, sw, ph, pw, dh, dw, Ho, Wo;
    unsigned P, Q;           // N Ho Wo, N H W
    int vec_a, vec_b;        // 16-byte loads allowed
    unsigned chunk;          // wgrad: positions per part (a multiple of LMP_S)
    int tiles_j;             // column tiles
};

// The row of the gathered map that tap (r, s) pairs with tile row (n, a, b), or -1 (padding, or a tap the stride does not divide).
//   fwd / wgrad: (a, b) = (ho sh - ph, wo sw - pw), the map is x        dgrad: (a, b) = (hi + ph, wi + pw), the map is dy
template <int MODE> __device__ __forceinline__ int cmp_src_row(const CmpP& p, int n, int a, int b, int r, int s) {
    if (MODE == CMP_DGRAD) {
        const int u = a - r * p.dh, v = b - s * p.dw;
        if (u < 0 || v < 0) return -1;
        const int ho = p.sh == 1 ? u : (int)((unsigned)u / (unsigned)p.sh), wo = p.sw == 1 ? v : (int)((unsigned)v / (unsigned)p.sw);
        if (ho * p.sh != u || wo * p.sw != v || ho >= p.Ho || wo >= p.Wo) return -1;
        return (n * p.Ho + ho) * p.Wo + wo;
    } else {
        const int hi = a + r * p.dh, wi = b + s * p.dw;
        if ((unsigned)hi >= (unsigned)p.H || (unsigned)wi >= (unsigned)p.W) return -1;
        return (n * p.H + hi) * p.W + wi;
    }
}

// one chunk of 4 consecutive floats at element `col` of row `src` (pitch `ld`; col + j < ld is checked), zeros where src < 0
__device__ __forceinline__ float4 cmp_load4(brsrc_t rs, int src, int ld, int col, bool vec) {
    const unsigned off = ((unsigned)src * (unsigned)ld + (unsigned)col) * 4u;        // below 2^31: the host checks the map's bytes
    const bool rok = src >= 0;
    float4 v;
    if (vec) {
        v = buf_load_f4(rs, (rok && col < ld) ? off : BUF_OOB);                      // ld % 4 == 0: a chunk is all in or all out
    } else {
        v.x = buf_load_f1(rs, (rok && col + 0 < ld) ? off : BUF_OOB);
        v.y = buf_load_f1(rs, (rok && col + 1 < ld) ? off + 4 : BUF_OOB);
        v.z = buf_load_f1(rs, (rok && col + 2 < ld) ? off + 8 : BUF_OOB);
        v.w = buf_load_f1(rs, (rok && col + 3 < ld) ? off + 12 : BUF_OOB);
    }
    return v;
}

// fwd / dgrad: lmp_gload<false>'s patch (chunk c = t + 256 u -> tile row c >> 3, reduction elements c0 + 4 (c & 7) .. + 3) with each
// row gathered: rn / ra / rb hold (n, a, b) of this thread's four tile rows, rn < 0 for a row past the tensor.
template <int MODE>
__device__ __forceinline__ void cmp_gload_rows(float4 (&v)[4], brsrc_t rs, const CmpP& p, const int (&rn)[4], const int (&ra)[4],
                                               const int (&rb)[4], int r, int s, int c0, int ld, bool vec, int t) {
    const int col = c0 + 4 * (t & 7);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int src = rn[u] < 0 ? -1 : cmp_src_row<MODE>(p, rn[u], ra[u], rb[u], r, s);
        v[u] = cmp_load4(rs, src, ld, col, vec);
    }
}

// wgrad: lmp_gload<true>'s patch (chunk c = t + 256 u -> reduction row c >> 5, columns 4 (c & 31) .. + 3) with each reduction row the
// input pixel that tap (r, s) pairs with output position pos0 + (c >> 5); positions from `pend` on belong to the next part.
__device__ __forceinline__ void cmp_gload_red(float4 (&v)[4], brsrc_t rs, const CmpP& p, unsigned pos0, unsigned pend, int r, int s, int j0,
                                              bool vec, int t) {
    const int col = j0 + 4 * (t & 31);
    const unsigned hw = (unsigned)(p.Ho * p.Wo);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const unsigned pos = pos0 + (unsigned)((t >> 5) + 8 * u);
        int src = -1;
        if (pos < pend) {
            const unsigned n = pos / hw, rem = pos - n * hw, ho = rem / (unsigned)p.Wo, wo = rem - ho * (unsigned)p.Wo;
            src = cmp_src_row<CMP_FWD>(p, (int)n, (int)ho * p.sh - p.ph, (int)wo * p.sw - p.pw, r, s);
        }
        v[u] = cmp_load4(rs, src, p.C, col, vec);
    }
}

template <int MODE> __global__ __launch_bounds__(256) void cmp_kernel(const CmpP p) {
    constexpr bool TA = MODE == CMP_WGRAD;            // A = the row operand of the product, B = the column operand
    constexpr bool TB = MODE != CMP_FWD;
    __shared__ __attribute__((aligned(16))) char lds[2][2][LMP_IMG];
    const int t = threadIdx.x;
    const int taps = p.R * p.S;
    const brsrc_t rs_g = make_brsrc(p.a);

    // ---- the tile
    unsigned i0;             // first output row
    int j0, tap = 0;         // first output column; wgrad: the tile's tap
    const unsigned I = MODE == CMP_FWD ? p.P : MODE == CMP_DGRAD ? p.Q : (unsigned)p.K;
    const int J = MODE == CMP_FWD ? p.K : p.C;
    if (MODE == CMP_WGRAD) {
        const unsigned tc = blockIdx.x % (unsigned)p.tiles_j, rest = blockIdx.x / (unsigned)p.tiles_j;
        tap = (int)(rest % (unsigned)taps);
        i0 = (rest / (unsigned)taps) * LMP_T;
        j0 = (int)tc * LMP_T;
    } else {
        i0 = (blockIdx.x / (unsigned)p.tiles_j) * LMP_T;
        j0 = (int)(blockIdx.x % (unsigned)p.tiles_j) * LMP_T;
    }
    const int rows_i = (int)(I - i0 < (unsigned)LMP_T ? I - i0 : (unsigned)LMP_T), rows_j = J - j0 < LMP_T ? J - j0 : LMP_T;

    // ---- the reduction
    const int red = MODE == CMP_FWD ? p.C : p.K;                      // fwd / dgrad: elements per tap
    const int chunks = (red + LMP_S - 1) / LMP_S;
    unsigned pbeg = 0, pend = 0;                                      // wgrad: this part's positions
    int steps;
    if (MODE == CMP_WGRAD) {
        pbeg = blockIdx.y * p.chunk;
        pend = p.P - pbeg < p.chunk ? p.P : pbeg + p.chunk;
        steps = (int)((pend - pbeg + LMP_S - 1) / LMP_S);
    } else {
        steps = taps * chunks;
    }

    // fwd / dgrad: this thread's four gathered tile rows (t >> 3) + 32 u, decoded once
    int rn[4], ra[4], rb[4];
    if (MODE != CMP_WGRAD) {
        const unsigned w_ = MODE == CMP_FWD ? (unsigned)p.Wo : (unsigned)p.W, hw = w_ * (MODE == CMP_FWD ? (unsigned)p.Ho : (unsigned)p.H);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int row = (t >> 3) + 32 * u;
            const unsigned pos = i0 + (unsigned)row;
            const unsigned n = pos / hw, rem = pos - n * hw, h = rem / w_, w = rem - h * w_;
            rn[u] = row < rows_i ? (int)n : -1;
            ra[u] = MODE == CMP_FWD ? (int)h * p.sh - p.ph : (int)h + p.ph;
            rb[u] = MODE == CMP_FWD ? (int)w * p.sw - p.pw : (int)w + p.pw;
        }
    }
    const int wtap_r = tap / p.S, wtap_s = tap - wtap_r * p.S;        // wgrad's tap

    int g_r = 0, g_s = 0, g_c0 = 0;              // fwd / dgrad: the (tap, chunk) the next load stages; lmp_reduce calls in step order
    int g_step = 0;                              // wgrad: the step it stages
    f32x16 acc[2][2];
    lmp_reduce<TA, TB>(acc, lds, steps, t, [&](float4 (&va)[4], float4 (&vb)[4]) {
        if (MODE == CMP_FWD) {
            const int left = red - g_c0 < LMP_S ? red - g_c0 : LMP_S;
            cmp_gload_rows<CMP_FWD>(va, rs_g, p, rn, ra, rb, g_r, g_s, g_c0, p.C, p.vec_a, t);
            lmp_gload<false>(vb, p.b + (long long)j0 * taps * p.C, (long long)taps * p.C, p.vec_b, rows_j, (g_r * p.S + g_s) * p.C + g_c0, left, t);
        } else if (MODE == CMP_DGRAD) {
            const int left = red - g_c0 < LMP_S ? red - g_c0 : LMP_S;
            cmp_gload_rows<CMP_DGRAD>(va, rs_g, p, rn, ra, rb, g_r, g_s, g_c0, p.K, p.vec_a, t);
            lmp_gload<true>(vb, p.b + ((long long)g_c0 * taps + (g_r * p.S + g_s)) * p.C + j0, (long long)taps * p.C, p.vec_b, rows_j, 0, left, t);
        } else {
            const unsigned r0 = pbeg + (unsigned)g_step * LMP_S;
            const int left = (int)(pend - r0 < (unsigned)LMP_S ? pend - r0 : (unsigned)LMP_S);
            lmp_gload<true>(va, p.b + (long long)r0 * p.K + i0, p.K, p.vec_b, rows_i, 0, left, t);
            cmp_gload_red(vb, rs_g, p, r0, pend, wtap_r, wtap_s, j0, p.vec_a, t);
        }
        ++g_step;
        g_c0 += LMP_S;
        if (g_c0 >= red) {
            g_c0 = 0;
            if (++g_s == p.S) { g_s = 0; ++g_r; }
        }
    });

    // fwd / dgrad: c[i][J]; wgrad: the tile's tap of dw[k][taps][C], in part blockIdx.y
    const long long ldc = MODE == CMP_WGRAD ? (long long)taps * p.C : (long long)J;
    float* cbase = p.c + (MODE == CMP_WGRAD ? (long long)blockIdx.y * p.K * ldc + (long long)tap * p.C : 0LL);
    lmp_store_tile(acc, cbase + (long long)i0 * ldc, (unsigned)ldc, rows_i, j0, J, MODE == CMP_FWD ? p.bias : nullptr, t);
}

// the gathered map is addressed from ONE descriptor at its base with 32-bit byte offsets
constexpr long long CMP_MAX_MAP_ELEMS = (1LL << 29) - 4;

struct CmpGeom {
    int N, H, W, C, K, R, S, sh, sw, ph, pw, dh, dw, Ho, Wo;
    long long P, Q;
};

// the argument checks the three entries share; fills Ho / Wo / P / Q
int cmp_geom(const char* who, CmpGeom& g) {
    MV_CHECK_ARG(g.N > 0 && g.H > 0 && g.W > 0 && g.C > 0 && g.K > 0 && g.R > 0 && g.S > 0, "%s: non-positive dimension", who);
    MV_CHECK_ARG(g.sh > 0 && g.sw > 0 && g.dh > 0 && g.dw > 0 && g.ph >= 0 && g.pw >= 0, "%s: bad stride / padding / dilation", who);
    const long long eh = (long long)g.H + 2LL * g.ph - (long long)g.dh * (g.R - 1) - 1, ew = (long long)g.W + 2LL * g.pw - (long long)g.dw * (g.S - 1) - 1;
    MV_CHECK_ARG(eh >= 0 && ew >= 0, "%s: empty output (the dilated filter is larger than the padded map)", who);
    g.Ho = (int)(eh / g.sh) + 1;
    g.Wo = (int)(ew / g.sw) + 1;
    g.P = (long long)g.N * g.Ho * g.Wo;
    g.Q = (long long)g.N * g.H * g.W;
    // the padded coordinates of cmp_src_row stay in int
    MV_CHECK_ARG((long long)g.H + g.ph + (long long)g.R * g.dh < (1LL << 30) && (long long)g.W + g.pw + (long long)g.S * g.dw < (1LL << 30),
                 "%s: padded map edge above 2^30", who);
    MV_CHECK_ARG(g.C <= LMP_MAX_DIM && g.K <= LMP_MAX_DIM && (long long)g.R * g.S * g.C <= LMP_MAX_DIM,
                 "%s: C = %d / K = %d / R S C = %lld above %d", who, g.C, g.K, (long long)g.R * g.S * g.C, LMP_MAX_DIM);
    if (g.Q * g.C > CMP_MAX_MAP_ELEMS || g.P * g.K > CMP_MAX_MAP_ELEMS) {
        set_error("%s: a map of %lld / %lld elements is beyond the kernel's 32-bit offsets (at most %lld)", who, g.Q * g.C, g.P * g.K,
                  CMP_MAX_MAP_ELEMS);
        return MV_E_UNSUPPORTED;
    }
    return MV_OK;
}

CmpP cmp_params(const CmpGeom& g) {
    CmpP p = {};
    p.H = g.H; p.W = g.W; p.C = g.C; p.K = g.K; p.R = g.R; p.S = g.S; p.sh = g.sh; p.sw = g.sw; p.ph = g.ph; p.pw = g.pw; p.dh = g.dh; p.dw = g.dw;
    p.Ho = g.Ho; p.Wo = g.Wo;
    p.P = (unsigned)g.P; p.Q = (unsigned)g.Q;
    p.chunk = 0;
    return p;
}

}  // namespace
}  // namespace mv

extern "C" {

using namespace mv;

int mv_conv2d_mp_fwd(const float* x, const float* w, const float* bias, float* y, int N, int H, int W, int C, int K, int R, int S, int sh,
                     int sw, int ph, int pw, int dh, int dw, mv_stream_t stream) {
    MV_CHECK_ARG(x && w && y, "conv2d_mp_fwd: null pointer");
    CmpGeom g = {N, H, W, C, K, R, S, sh, sw, ph, pw, dh, dw, 0, 0, 0, 0};
    const int rc = cmp_geom("conv2d_mp_fwd", g);
    if (rc != MV_OK) return rc;
    CmpP p = cmp_params(g);
    p.a = x; p.b = w; p.bias = bias; p.c = y;
    p.vec_a = lmp_vec_ok(x, C);
    p.vec_b = lmp_vec_ok(w, C);                                   // a tap's channels start at a multiple of C
    p.tiles_j = (K + LMP_T - 1) / LMP_T;
    const long long tiles = ((g.P + LMP_T - 1) / LMP_T) * p.tiles_j;
    set_kernel_name("conv_mp_fwd_bf16");
    hipLaunchKernelGGL((cmp_kernel<CMP_FWD>), dim3((unsigned)tiles), dim3(256), 0, (hipStream_t)stream, p);
    MV_LAUNCH_CHECK();
    return MV_OK;
}

int mv_conv2d_mp_dgrad(const float* dy, const float* w, float* dx, int N, int H, int W, int C, int K, int R, int S, int sh, int sw, int ph,
                       int pw, int dh, int dw, mv_stream_t stream) {
    MV_CHECK_ARG(dy && w && dx, "conv2d_mp_dgrad: null pointer");
    CmpGeom g = {N, H, W, C, K, R, S, sh, sw, ph, pw, dh, dw, 0, 0, 0, 0};
    const int rc = cmp_geom("conv2d_mp_dgrad", g);
    if (rc != MV_OK) return rc;
    CmpP p = cmp_params(g);
    p.a = dy; p.b = w; p.bias = nullptr; p.c = dx;
    p.vec_a = lmp_vec_ok(dy, K);
    p.vec_b = lmp_vec_ok(w, C);                                   // rows of R S C floats, the tile's columns start at tap C + j0
    p.tiles_j = (C + LMP_T - 1) / LMP_T;
    const long long tiles = ((g.Q + LMP_T - 1) / LMP_T) * p.tiles_j;
    set_kernel_name("conv_mp_dgrad_bf16");
    hipLaunchKernelGGL((cmp_kernel<CMP_DGRAD>), dim3((unsigned)tiles), dim3(256), 0, (hipStream_t)stream, p);
    MV_LAUNCH_CHECK();
    return MV_OK;
}

int mv_conv2d_mp_wgrad(const float* x, const float* dy, float* dw_krsc, int N, int H, int W, int C, int K, int R, int S, int sh, int sw,
                       int ph, int pw, int dh, int dw, mv_stream_t stream) {
    MV_CHECK_ARG(x && dy && dw_krsc, "conv2d_mp_wgrad: null pointer");
    CmpGeom g = {N, H, W, C, K, R, S, sh, sw, ph, pw, dh, dw, 0, 0, 0, 0};
    const int rc = cmp_geom("conv2d_mp_wgrad", g);
    if (rc != MV_OK) return rc;
    const long long out_elems = (long long)K * R * S * C;
    const long long tiles = (((long long)K + LMP_T - 1) / LMP_T) * R * S * (((long long)C + LMP_T - 1) / LMP_T);
    if (tiles >= (1LL << 31)) {
        set_error("conv2d_mp_wgrad: %lld output tiles do not fit the grid", tiles);
        return MV_E_UNSUPPORTED;
    }
    const LmpSplit sp = lmp_wgrad_split(tiles, g.P, out_elems, (hipStream_t)stream, dw_krsc);        // the P positions split over blocks
    CmpP p = cmp_params(g);
    p.a = x; p.b = dy; p.bias = nullptr; p.c = sp.part;
    p.vec_a = lmp_vec_ok(x, C);
    p.vec_b = lmp_vec_ok(dy, K);
    p.chunk = (unsigned)sp.chunk;
    p.tiles_j = (C + LMP_T - 1) / LMP_T;
    set_kernel_name(sp.split > 1 ? "conv_mp_wgrad_split_bf16" : "conv_mp_wgrad_bf16");
    hipLaunchKernelGGL((cmp_kernel<CMP_WGRAD>), dim3((unsigned)tiles, (unsigned)sp.split), dim3(256), 0, (hipStream_t)stream, p);
    if (sp.split > 1) sum_parts((hipStream_t)stream, sp.part, dw_krsc, out_elems, (int)sp.split);
    MV_LAUNCH_CHECK();
    return MV_OK;
}

}  // extern "C"
