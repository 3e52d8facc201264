// Weight-stationary streaming kernel for the memory-bound pointwise layers (1x1 stride-1 Conv2d and
// Linear with a short reduction: K <= 256), gfx950.
//
//   y[m, n] = act( scale[n] * sum_k x[m, k] * w[n, k] + shift[n] + res[m, n] ),   k contiguous in x and w
//
// These layers (ResNet-50: 64->256, 256->64, 128->512, 256->1024 ... at 56x56 .. 14x14) move >100 bytes
// per kFLOP: they are HBM-bound and were latency-starved in the tiled igemm kernel (2-3 TB/s): one k-tile
// per block means load -> compute -> store phases in series with nothing else in flight.  Here
//   * the block's weight slab W[BN][K] (<= 64 KB) is loaded into LDS ONCE and stays there;
//   * every wave owns whole 32-pixel tiles: its x operand is needed by no other wave, so it never
//     goes through LDS -- each lane loads its MFMA B-fragments (16 bytes) straight from HBM into VGPRs,
//     double buffered one tile ahead; the residual row chunks of the tile are fetched before its MFMAs;
//   * there is NO block barrier in the steady state: 8 waves per CU free-run over a grid-stride list of
//     pixel tiles, so loads, MFMAs and stores of different waves overlap continuously;
//   * the epilogue is the igemm one: fp32 scale/shift in the accumulator layout, transpose through a
//     wave-private LDS patch, then 16-byte-per-lane full-line NHWC stores;
//   * a block keeps as many 128-channel slabs of W as fit in LDS (`npass`) and runs them one after the other on
//     the SAME x fragments, so x is read once per block row instead of once per channel tile (Swin C=96 ->
//     288 / 384, ResNet 64 -> 256), and two pixel tiles are in flight per wave (two fragment sets, each refilled
//     a whole tile before its next use): with one 6 KB tile per wave in flight the K=96 layers were
//     latency-bound at 3.3 TB/s.
#include "mfma_common.h"

namespace mv {

struct StreamP {
    const bf16_t* x;
    const bf16_t* w;
    const float* scale;
    const float* shift;
    const void* residual;
    void* y;
    int M, K, N;          // rows, reduction, output channels
    int tiles_m, act, wpitch;
    int npass;            // 128-channel slabs of W resident per block (channel tiles blockIdx.y*npass ...)
    const void* xraw;     // LN mode: the un-normalised rows (fp32 or bf16), normalised in registers on the way in
    float eps;
};

template <typename OutT> struct SRes8;
template <> struct SRes8<bf16_t> {
    uint4 u;
    __device__ __forceinline__ void load(const bf16_t* p) { u = *(const uint4*)p; }
    __device__ __forceinline__ void add_to(float* v) const {
        const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            v[2 * e] += __uint_as_float(w[e] << 16);
            v[2 * e + 1] += __uint_as_float(w[e] & 0xffff0000u);
        }
    }
};
template <> struct SRes8<float> {
    float4 a, b;
    __device__ __forceinline__ void load(const float* p) { a = *(const float4*)p; b = *(const float4*)(p + 4); }
    __device__ __forceinline__ void add_to(float* v) const {
        v[0] += a.x; v[1] += a.y; v[2] += a.z; v[3] += a.w; v[4] += b.x; v[5] += b.y; v[6] += b.z; v[7] += b.w;
    }
};

// TN = 32-channel MFMA tiles per wave and pass (BN = 32*TN), KC = K/16 MFMA k-steps, WAVES per block.
// LN: the rows arrive un-normalised in XT (the fp32 residual stream, or bf16); every lane holds half of its row, so the
// LayerNorm statistics are two cross-half shuffles and (x - mean) * rstd becomes the bf16 B fragment directly (the affine
// part of the LayerNorm is folded into w / shift by the caller).  Saves the separate LayerNorm launch and its round trip.
// KPAD: the reduction p.K is a multiple of 8 but not of 16 (24, 40, 72, 120 ... : MobileNet / EfficientNet / RegNet widths): the
// last k-step is half empty -- its upper 8 channels are zero in the LDS weight rows and in the fragments (masked loads).
template <int TN, int KC, int WAVES, typename OutT, bool LN = false, typename XT = bf16_t, bool KPAD = false>
__global__ __launch_bounds__(WAVES * 64) void stream1x1_kernel(const StreamP p) {
    constexpr int BN = 32 * TN;
    constexpr int EPITCH = 64 * 4 + 16;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int rows = p.npass * BN;                              // weight rows resident in this block
    char* wl = smem;                                            // [rows][wpitch]
    float* sct = (float*)(smem + rows * p.wpitch);              // [2][rows]: scale, shift of the block's channels
    char* ep = (char*)(sct + 2 * rows) + wave * (32 * EPITCH);  // wave-private epilogue patch
    const int nb = blockIdx.y * rows;                           // first channel of the block
    const int K = KPAD ? p.K : KC * 16;                         // row pitch of x and w in memory

    // ---- weight slab + scale / shift -> LDS (once).  16-byte chunks, zero rows past N.
    {
        constexpr int CH = KC * 2;                              // 16-byte chunks per row
        for (int base = 0; base < rows * CH; base += WAVES * 64 * 4) {
            uint4 v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int i = base + j * WAVES * 64 + tid;
                const int row = i / CH, ch = i - row * CH;
                const int n = nb + row;
                const bool ok = i < rows * CH && n < p.N && (!KPAD || ch * 8 < K);
                v[j] = *(const uint4*)(p.w + (ok ? (long long)n * K + ch * 8 : 0));
                if (!ok) v[j] = make_uint4(0, 0, 0, 0);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int i = base + j * WAVES * 64 + tid;
                const int row = i / CH, ch = i - row * CH;
                if (i < rows * CH) *(uint4*)(wl + row * p.wpitch + ch * 16) = v[j];
            }
        }
        for (int i = tid; i < rows; i += WAVES * 64) {
            const int n = nb + i;
            sct[i] = (p.scale && n < p.N) ? p.scale[n] : 1.f;
            sct[rows + i] = (p.shift && n < p.N) ? p.shift[n] : 0.f;
        }
    }
    __syncthreads();

    const int fr = lane & 31, fh = lane >> 5;
    const int gw = blockIdx.x * WAVES + wave, nw = gridDim.x * WAVES;
    OutT* y = (OutT*)p.y;
    const OutT* res = (const OutT*)p.residual;
    const char* wfrag = wl + fr * p.wpitch + fh * 16;           // + (pass*BN + a*32)*wpitch + kk*32

    auto load_x = [&](uint4* xf, int tile) {
        int m = tile * 32 + fr;
        m = m < p.M ? m : p.M - 1;                              // clamp: rows past the end are never stored
        const bf16_t* src = p.x + (long long)m * K + fh * 8;
#pragma unroll
        for (int kk = 0; kk < KC; ++kk) {
            if (KPAD && kk == KC - 1) {                         // the half-empty last step: lanes of the upper half hold zeros
                const bool in = fh == 0;
                xf[kk] = *(const uint4*)(src + (in ? kk * 16 : 0));
                if (!in) xf[kk] = make_uint4(0, 0, 0, 0);
            } else {
                xf[kk] = *(const uint4*)(src + kk * 16);
            }
        }
    };
    auto load_res = [&](SRes8<OutT> (*rr)[4], int tile, int n0) {
#pragma unroll
        for (int c = 0; c < TN / 2; ++c)
#pragma unroll
            for (int pass = 0; pass < 4; ++pass) {
                const int m = tile * 32 + pass * 8 + (lane >> 3);
                const int n = n0 + c * 64 + (lane & 7) * 8;
                const bool ok = m < p.M && n < p.N;
                rr[c][pass].load(res + (ok ? (long long)m * p.N + n : 0));
            }
    };

    // One pixel tile: every resident channel slab on the same fragments, then the fragments are refilled for the
    // tile two strides ahead (`refill`), a whole tile of work before they are needed again.
    SRes8<OutT> rr[TN / 2][4];
    auto run_tile = [&](uint4* xf, int tile, int refill) {
        for (int ps = 0; ps < p.npass; ++ps) {
            const int n0 = nb + ps * BN;
            if (n0 >= p.N) break;
            if (res) load_res(rr, tile, n0);                   // flies under this slab's MFMAs
            f32x16 acc[TN];
#pragma unroll
            for (int a = 0; a < TN; ++a)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[a][e] = 0.f;
            const char* wf = wfrag + (size_t)ps * BN * p.wpitch;
#pragma unroll
            for (int kk = 0; kk < KC; ++kk) {
#pragma unroll
                for (int a = 0; a < TN; ++a) {
                    const uint4 av = *(const uint4*)(wf + a * 32 * p.wpitch + kk * 32);
                    acc[a] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, av),
                                                                     __builtin_bit_cast(bf16x8, xf[kk]), acc[a], 0, 0, 0);
                }
            }
            if ((ps == p.npass - 1 || n0 + BN >= p.N) && refill < p.tiles_m) load_x(xf, refill);
            // epilogue: accumulator layout -> LDS patch -> row-major full lines
#pragma unroll
            for (int c = 0; c < TN / 2; ++c) {
#pragma unroll
                for (int a2 = 0; a2 < 2; ++a2) {
                    const int a = 2 * c + a2;
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const int nl = a2 * 32 + 8 * g + 4 * fh;
                        float4 v = make_float4(acc[a][4 * g], acc[a][4 * g + 1], acc[a][4 * g + 2], acc[a][4 * g + 3]);
                        *(float4*)(ep + fr * EPITCH + nl * 4) = v;
                    }
                }
                wave_lds_fence();                                  // patch written by all lanes -> read back row-major
                const int c8 = lane & 7;
                const int nloc = ps * BN + c * 64 + c8 * 8;        // my 8 channels inside the block's slab set
                const float4 s0 = *(const float4*)(sct + nloc), s1 = *(const float4*)(sct + nloc + 4);
                const float4 h0 = *(const float4*)(sct + rows + nloc), h1 = *(const float4*)(sct + rows + nloc + 4);
                const float scv[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
                const float shv[8] = {h0.x, h0.y, h0.z, h0.w, h1.x, h1.y, h1.z, h1.w};
#pragma unroll
                for (int pass = 0; pass < 4; ++pass) {
                    const int row = pass * 8 + (lane >> 3);
                    const int m = tile * 32 + row;
                    const int n = n0 + c * 64 + c8 * 8;
                    const float4 lo = *(const float4*)(ep + row * EPITCH + c8 * 32);
                    const float4 hi = *(const float4*)(ep + row * EPITCH + c8 * 32 + 16);
                    if (m < p.M && n < p.N) {
                        float v[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
                        for (int e = 0; e < 8; ++e) v[e] = fmaf(v[e], scv[e], shv[e]);
                        if (res) rr[c][pass].add_to(v);
                        if (p.act == MV_ACT_RELU) {
#pragma unroll
                            for (int e = 0; e < 8; ++e) v[e] = fmaxf(v[e], 0.f);
                        } else if (p.act == MV_ACT_GELU_TANH) {
#pragma unroll
                            for (int e = 0; e < 8; ++e) v[e] = gelu_tanh_f(v[e]);
                        } else if (p.act > MV_ACT_GELU_TANH) {     // hard_swish / hard_sigmoid / sigmoid / silu (MobileNetV3, EfficientNet)
#pragma unroll
                            for (int e = 0; e < 8; ++e) v[e] = apply_act_rt(v[e], p.act);
                        }
                        Out8<OutT>::st(y + (long long)m * p.N + n, v);
                    }
                }
                wave_lds_fence();                                  // before the patch is overwritten by the next chunk
            }
        }
    };

    if constexpr (LN) {
        // one raw row set in flight (fetched a whole tile ahead), normalised into the fragment set right before use
        const XT* xr = (const XT*)p.xraw;
        float raw[KC][8];
        auto load_raw = [&](int t) {
            int m = t * 32 + fr;
            m = m < p.M ? m : p.M - 1;
            const XT* src = xr + (long long)m * K + fh * 8;
#pragma unroll
            for (int kk = 0; kk < KC; ++kk) {
                if constexpr (sizeof(XT) == 4) {
                    const float4 a = *(const float4*)(src + kk * 16), b = *(const float4*)(src + kk * 16 + 4);
                    raw[kk][0] = a.x; raw[kk][1] = a.y; raw[kk][2] = a.z; raw[kk][3] = a.w;
                    raw[kk][4] = b.x; raw[kk][5] = b.y; raw[kk][6] = b.z; raw[kk][7] = b.w;
                } else {
                    const uint4 u = *(const uint4*)(src + kk * 16);
                    const uint32_t w4[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        raw[kk][2 * e] = __uint_as_float(w4[e] << 16);
                        raw[kk][2 * e + 1] = __uint_as_float(w4[e] & 0xffff0000u);
                    }
                }
            }
        };
        uint4 xa[KC];
        int tile = gw;
        constexpr bool AHEAD = KC <= 6;                          // K = 192: 96 raw + 48 fragment registers do not fit twice
        if (AHEAD && tile < p.tiles_m) load_raw(tile);
        for (; tile < p.tiles_m; tile += nw) {
            if (!AHEAD) load_raw(tile);
            float s = 0.f;
#pragma unroll
            for (int kk = 0; kk < KC; ++kk)
#pragma unroll
                for (int e = 0; e < 8; ++e) s += raw[kk][e];
            s += __shfl_xor(s, 32);
            const float mean = s * (1.0f / K);
            float q = 0.f;
#pragma unroll
            for (int kk = 0; kk < KC; ++kk)
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float d = raw[kk][e] - mean;
                    q = fmaf(d, d, q);
                }
            q += __shfl_xor(q, 32);
            const float rstd = rsqrtf(q * (1.0f / K) + p.eps);
#pragma unroll
            for (int kk = 0; kk < KC; ++kk) {
                xa[kk].x = pack_bf2((raw[kk][0] - mean) * rstd, (raw[kk][1] - mean) * rstd);
                xa[kk].y = pack_bf2((raw[kk][2] - mean) * rstd, (raw[kk][3] - mean) * rstd);
                xa[kk].z = pack_bf2((raw[kk][4] - mean) * rstd, (raw[kk][5] - mean) * rstd);
                xa[kk].w = pack_bf2((raw[kk][6] - mean) * rstd, (raw[kk][7] - mean) * rstd);
            }
            if (AHEAD && tile + nw < p.tiles_m) load_raw(tile + nw);
            run_tile(xa, tile, p.tiles_m);                       // no in-kernel refill of the fragment set
        }
        return;
    }
    constexpr bool X2 = KC <= 8;                                // two fragment sets: 2 x KC x 4 VGPRs (K = 256 would spill)
    uint4 xa[KC], xb[X2 ? KC : 1];
    int tile = gw;
    if (tile < p.tiles_m) load_x(xa, tile);
    if constexpr (X2) {
        if (tile + nw < p.tiles_m) load_x(xb, tile + nw);
        for (; tile < p.tiles_m; tile += 2 * nw) {
            run_tile(xa, tile, tile + 2 * nw);
            if (tile + nw < p.tiles_m) run_tile(xb, tile + nw, tile + 3 * nw);
        }
    } else {
        for (; tile < p.tiles_m; tile += nw) run_tile(xa, tile, tile + nw);
    }
}

template <int TN, int KC, typename OutT, bool LN = false, typename XT = bf16_t, bool KPAD = false>
static int stream_go(StreamP& p, int tiles_n, hipStream_t st) {
    constexpr int WAVES = 8;
    // as many channel slabs per block as LDS holds next to the epilogue patches (160 KB per CU, one block per CU)
    const size_t slab = (size_t)32 * TN * p.wpitch + (size_t)2 * 32 * TN * 4, patches = (size_t)WAVES * 32 * (64 * 4 + 16);
    int npass = (int)((160 * 1024 - 1024 - patches) / slab);
    if (npass > tiles_n) npass = tiles_n;
    if (npass < 1) npass = 1;
    p.npass = npass;
    const int gy = (tiles_n + npass - 1) / npass;
    const size_t smem = slab * npass + patches;
    int gx = 256 / gy;                                        // ~one block per CU in total
    if (gx < 1) gx = 1;
    const int need = (p.tiles_m + WAVES - 1) / WAVES;
    if (gx > need) gx = need;
    dim3 grid(gx, gy), block(WAVES * 64);
    auto kern = stream1x1_kernel<TN, KC, WAVES, OutT, LN, XT, KPAD>;
    if (smem > 48 * 1024)
        MV_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
    hipLaunchKernelGGL(kern, grid, block, smem, st, p);
    MV_LAUNCH_CHECK();
    return MV_OK;
}

static int stream1x1_ln_supported(long long M, int C, int K, int x_dtype, int out_dtype) {
    // K = 192 works (flag "ln_stream_192") but loses: only one 128-channel weight slab fits in LDS next to the epilogue patches,
    // so 5-6 blocks re-read AND re-normalise every row (measured 46 us vs 14 + 29.5 us for LayerNorm + Linear at 50 176 x 192 -> 576)
    const bool c_ok = C == 96 || (C == 192 && get_flag("ln_stream_192"));
    return (x_dtype == MV_F32 || x_dtype == MV_BF16) && out_dtype == MV_BF16 && c_ok && K % 8 == 0 && K > 64 &&
           M >= 8192 && M < (1ll << 31) - 64 && !get_flag("no_ln_stream");
}

// y = act(w . n(x) + shift): rows normalised on the way in (LayerNorm with its affine folded into w / shift by the caller)
static int stream1x1_ln_launch(const void* x, const void* w, const float* shift, void* y, long long M, int C, int K, float eps,
                               int act, int x_dtype, hipStream_t st) {
    StreamP p;
    p.x = nullptr; p.xraw = x; p.eps = eps;
    p.w = (const bf16_t*)w; p.scale = nullptr; p.shift = shift; p.residual = nullptr; p.y = y;
    p.M = (int)M; p.K = C; p.N = K;
    p.tiles_m = (int)((M + 31) / 32);
    p.act = act;
    p.wpitch = C * 2 + 16;
    const int tiles_n = (K + 127) / 128;
    char name[64];
    snprintf(name, sizeof(name), "stream1x1_ln_%s_k%d", x_dtype == MV_F32 ? "f32in" : "bf16in", C);
    set_kernel_name(name);
    if (x_dtype == MV_F32)
        return C == 96 ? stream_go<4, 6, bf16_t, true, float>(p, tiles_n, st) : stream_go<4, 12, bf16_t, true, float>(p, tiles_n, st);
    return C == 96 ? stream_go<4, 6, bf16_t, true, bf16_t>(p, tiles_n, st) : stream_go<4, 12, bf16_t, true, bf16_t>(p, tiles_n, st);
}

int stream1x1_launch(const void* x, const void* w, const float* scale, const float* shift, const void* residual,
                     void* y, long long M, int C, int K, int act, int out_dtype, hipStream_t st) {
    StreamP p;
    p.xraw = nullptr; p.eps = 0.f;
    p.x = (const bf16_t*)x; p.w = (const bf16_t*)w; p.scale = scale; p.shift = shift; p.residual = residual; p.y = y;
    p.M = (int)M; p.K = C; p.N = K;
    p.tiles_m = (int)((M + 31) / 32);
    p.act = act;
    p.wpitch = ((C + 15) / 16) * 32 + 16;                      // odd number of 16-byte slots: conflict-free fragments
    const bool f32o = out_dtype == MV_F32;
    const int bn = (K <= 64) ? 64 : 128;
    const int tiles_n = (K + bn - 1) / bn;
#define GO(TN_, KC_)                                                              \
    return f32o ? stream_go<TN_, KC_, float>(p, tiles_n, st) : stream_go<TN_, KC_, bf16_t>(p, tiles_n, st)
#define GOP(TN_, KC_)                                                             \
    return f32o ? stream_go<TN_, KC_, float, false, bf16_t, true>(p, tiles_n, st)  \
                : stream_go<TN_, KC_, bf16_t, false, bf16_t, true>(p, tiles_n, st)
#define GOK(TN_)                                                   \
    if (C % 16) {                                                  \
        switch ((C + 15) / 16) {                                   \
            case 2: GOP(TN_, 2);                                   \
            case 3: GOP(TN_, 3);                                   \
            case 4: GOP(TN_, 4);                                   \
            case 5: GOP(TN_, 5);                                   \
            case 6: GOP(TN_, 6);                                   \
            case 7: GOP(TN_, 7);                                   \
            case 8: GOP(TN_, 8);                                   \
            case 9: GOP(TN_, 9);                                   \
            case 10: GOP(TN_, 10);                                 \
            case 11: GOP(TN_, 11);                                 \
            case 12: GOP(TN_, 12);                                 \
            case 13: GOP(TN_, 13);                                 \
            default: GOP(TN_, 15);                                 \
        }                                                          \
    }                                                              \
    switch (C / 16) {                                              \
        case 1: GO(TN_, 1);                                        \
        case 2: GO(TN_, 2);                                        \
        case 3: GO(TN_, 3);                                        \
        case 4: GO(TN_, 4);                                        \
        case 5: GO(TN_, 5);                                        \
        case 6: GO(TN_, 6);                                        \
        case 7: GO(TN_, 7);                                        \
        case 8: GO(TN_, 8);                                        \
        case 9: GO(TN_, 9);                                        \
        case 10: GO(TN_, 10);                                      \
        case 11: GO(TN_, 11);                                      \
        case 12: GO(TN_, 12);                                      \
        case 13: GO(TN_, 13);                                      \
        case 14: GO(TN_, 14);                                      \
        case 15: GO(TN_, 15);                                      \
        default: GO(TN_, 16);                                      \
    }
    if (bn == 64) {
        GOK(2);
    }
    GOK(4);
#undef GOP
#undef GOK
#undef GO
}

}  // namespace mv

using namespace mv;

extern "C" {

int mv_ln_linear_supported(int64_t M, int N, int K, int x_dtype, int out_dtype) {
    return !get_flag("force_generic") && !get_flag("no_stream") && stream1x1_ln_supported(M, K, N, x_dtype, out_dtype);
}

int mv_ln_linear_fwd(const void* x, const void* w, const float* bias, void* y, int64_t M, int N, int K, float eps, int act,
                     int x_dtype, int out_dtype, mv_stream_t stream) {
    MV_CHECK_FUSED_ACT(act, "ln_linear");
    MV_CHECK_ARG(x && w && y, "ln_linear: NULL pointer");
    if (!mv_ln_linear_supported(M, N, K, x_dtype, out_dtype)) {
        set_error("ln_linear: unsupported configuration M=%lld N=%d K=%d (ask mv_ln_linear_supported first)", (long long)M, N, K);
        return MV_E_UNSUPPORTED;
    }
    return stream1x1_ln_launch(x, w, bias, y, M, K, N, eps, act, x_dtype, (hipStream_t)stream);
}

}  // extern "C"
