// SqueezeNet Fire module, expand half (reference squeezenet.py:45-53): expand1x1 + ReLU, expand3x3 (pad 1) + ReLU and the channel
// concatenation of the two in ONE launch.  NHWC bf16, fp32 accumulation on the matrix cores, gfx950.
//
//   y[m, n]      = relu( b1[n] + sum_{c<S}          W1[n][c]       t[m, c] )                       n < E1
//   y[m, E1 + n] = relu( b3[n] + sum_{r,s<3, c<S}   W3[n][c][r][s] t[b, h + r - 1, w + s - 1, c] ) n < E3     (zero padding)
//
// A 256-thread workgroup owns TM = 128 PT consecutive flattened pixels (13 x 13 maps fill the machine at batch size) and stages their
// flat range of t in LDS once (flat3x3.h: the range, the zero slot, the fragment order).  The k-step of 16 channels divides every S
// in {16, 32, 48, 64}, so nothing is padded.  A wave owns 32 PT pixels and walks every 64-channel pair of output tiles from the one
// LDS copy: the expand1x1 tiles reduce over the centre tap only (S / 16 steps), the expand3x3 tiles over the nine taps (9 S / 16
// steps), fully unrolled; every B fragment read from LDS feeds two MFMAs and every A fragment PT.
#include "flat3x3.h"

namespace mv {

namespace {

constexpr int FE_THREADS = 256;
constexpr int FE_LDS_MAX = 160 * 1024;
constexpr int FE_LDS_TWO = 64 * 1024;          // the 256-pixel tile is used while two workgroups still fit a CU

struct FireP {
    const bf16_t* t;       // [M][S]
    const uint4* w1;       // [E1 / 32][S / 16][64] fragments
    const float* b1;       // [E1] or null
    const uint4* w3;       // [E3 / 32][9 S / 16][64] fragments
    const float* b3;       // [E3] or null
    bf16_t* y;             // [M][E1 + E3]
    long long M;           // B * H * W
    int H, W, S, E1, E3;
    int row_b;             // LDS bytes per pixel slot: 2 S + 16
    int n_slots;           // TM + 2 W + 2 staged pixels; slot n_slots is the zero pixel
};

// one pair of 32-channel tiles x PT pixel tiles over NT taps (1: the centre tap, 9: all)
template <int PT, int KC, int NT>
__device__ __forceinline__ void fire_pair(const uint4* __restrict__ wf, const char* lds, const int (&off)[PT][9], f32x16 (&acc)[2][PT],
                                          const int lane) {
    constexpr int KS = NT * KC;
#pragma unroll
    for (int tp = 0; tp < NT; ++tp) {
        const int tap = NT == 1 ? 4 : tp;
#pragma unroll
        for (int kc = 0; kc < KC; ++kc) {
            const int ks = tp * KC + kc;
            const bf16x8 a0 = __builtin_bit_cast(bf16x8, wf[ks * 64 + lane]);
            const bf16x8 a1 = __builtin_bit_cast(bf16x8, wf[(KS + ks) * 64 + lane]);
#pragma unroll
            for (int q = 0; q < PT; ++q) {
                const bf16x8 b = __builtin_bit_cast(bf16x8, *(const uint4*)(lds + off[q][tap] + kc * 32));
                acc[0][q] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b, acc[0][q], 0, 0, 0);
                acc[1][q] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b, acc[1][q], 0, 0, 0);
            }
        }
    }
}

// bias + ReLU + store: the lane holds channels cb .. cb + 15 of pixel m (accumulator registers 0 .. 15 in that order)
__device__ __forceinline__ void fire_store(const f32x16& a, const float* bias, bf16_t* y, const long long m, const long long M,
                                           const int cb, const int Ctot) {
    if (m >= M || cb + 16 > Ctot) return;
    float bv[16];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const float4 b = bias ? *(const float4*)(bias + 4 * g) : make_float4(0.f, 0.f, 0.f, 0.f);
        bv[4 * g] = b.x; bv[4 * g + 1] = b.y; bv[4 * g + 2] = b.z; bv[4 * g + 3] = b.w;
    }
    uint32_t o[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = pack_bf2(fmaxf(a[2 * e] + bv[2 * e], 0.f), fmaxf(a[2 * e + 1] + bv[2 * e + 1], 0.f));
    uint4* dst = (uint4*)(y + m * Ctot + cb);
    dst[0] = make_uint4(o[0], o[1], o[2], o[3]);
    dst[1] = make_uint4(o[4], o[5], o[6], o[7]);
}

template <int PT, int KC>
__global__ __launch_bounds__(FE_THREADS) void fire_expand_kernel(const FireP p) {
    constexpr int TM = 128 * PT;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long m0 = (long long)blockIdx.x * TM;
    const int W = p.W, S = p.S;

    // ---- 1. the flat pixel range of t and the zero pixel to LDS; 2 KC 16-byte chunks per pixel
    flat_stage<FE_THREADS>(smem, p.t, S, 0, 2 * KC, m0, W, p.M, p.n_slots, p.row_b, tid);

    // ---- 2. the LDS byte offsets of the nine taps of this lane's pixels
    int off[PT][9];
    const int hh = lane >> 5;
#pragma unroll
    for (int q = 0; q < PT; ++q) flat_tap_offsets(off[q], (wave * PT + q) * 32 + (lane & 31), m0, p.M, p.H, W, p.n_slots, p.row_b, hh);
    __syncthreads();

    // ---- 3. every 64-channel pair of output tiles from the one copy: expand1x1 (centre tap), then expand3x3 (nine taps)
    const int Ctot = p.E1 + p.E3;
    const int P1 = p.E1 >> 6, P3 = p.E3 >> 6;
    for (int pr = 0; pr < P1 + P3; ++pr) {
        f32x16 acc[2][PT];
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int q = 0; q < PT; ++q)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[j][q][e] = 0.f;
        const bool three = pr >= P1;
        const int tile0 = 2 * (three ? pr - P1 : pr);               // first 32-channel tile of the pair inside its half
        if (three) fire_pair<PT, KC, 9>(p.w3 + (long long)tile0 * (9 * KC) * 64, smem, off, acc, lane);
        else fire_pair<PT, KC, 1>(p.w1 + (long long)tile0 * KC * 64, smem, off, acc, lane);
        const float* bias = three ? p.b3 : p.b1;
        const int half_off = three ? p.E1 : 0;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int n = (tile0 + j) * 32 + 16 * hh;               // first of the lane's 16 channels inside its half
#pragma unroll
            for (int q = 0; q < PT; ++q)
                fire_store(acc[j][q], bias ? bias + n : nullptr, p.y, m0 + (wave * PT + q) * 32 + (lane & 31), p.M, half_off + n, Ctot);
        }
    }
}

template <int PT, int KC>
int fire_go(FireP p, hipStream_t st) {
    static LdsAttrSite site;
    auto kern = fire_expand_kernel<PT, KC>;
    p.n_slots = 128 * PT + 2 * p.W + 2;
    const size_t smem = flat_lds_bytes(128 * PT, p.W, p.S);
    MV_HIP(site.ensure((const void*)kern, smem));
    const long long blocks = (p.M + 128 * PT - 1) / (128 * PT);
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(FE_THREADS), smem, st, p);
    MV_LAUNCH_CHECK();
    return MV_OK;
}

template <int PT>
int fire_go_kc(const FireP& p, hipStream_t st) {
    switch (p.S >> 4) {
        case 1: return fire_go<PT, 1>(p, st);
        case 2: return fire_go<PT, 2>(p, st);
        case 3: return fire_go<PT, 3>(p, st);
        default: return fire_go<PT, 4>(p, st);
    }
}

}  // namespace

}  // namespace mv

extern "C" {

int mv_fire_expand_supported(int S, int E1, int E3, int H, int W, int x_dtype, int y_dtype) {
    if (mv::get_flag("no_fire_expand") || mv::get_flag("force_generic")) return 0;
    if (x_dtype != MV_BF16 || y_dtype != MV_BF16) return 0;
    if (S != 16 && S != 32 && S != 48 && S != 64) return 0;
    if (E1 != E3 || (E1 != 64 && E1 != 128 && E1 != 192 && E1 != 256)) return 0;
    if (H < 1 || W < 1 || H > 4096 || W > 4096) return 0;
    return mv::flat_lds_bytes(128, W, S) <= (size_t)mv::FE_LDS_MAX;           // the tile and its halo rows have to fit LDS
}

int mv_fire_expand_fwd(const void* t, const void* w1_frag, const float* b1, const void* w3_frag, const float* b3, void* y, int B,
                       int H, int W, int S, int E1, int E3, int x_dtype, int y_dtype, mv_stream_t stream_) {
    using namespace mv;
    MV_CHECK_ARG(t && w1_frag && w3_frag && y, "mv_fire_expand_fwd: NULL argument");
    MV_CHECK_ARG(t != y, "mv_fire_expand_fwd: not in place");
    MV_CHECK_ARG(B >= 1, "mv_fire_expand_fwd: B=%d", B);
    if (!mv_fire_expand_supported(S, E1, E3, H, W, x_dtype, y_dtype)) {
        set_error("mv_fire_expand_fwd: unsupported S=%d E1=%d E3=%d H=%d W=%d x_dtype=%d y_dtype=%d (ask mv_fire_expand_supported first)",
                  S, E1, E3, H, W, x_dtype, y_dtype);
        return MV_E_UNSUPPORTED;
    }
    FireP p;
    p.t = (const bf16_t*)t; p.w1 = (const uint4*)w1_frag; p.b1 = b1; p.w3 = (const uint4*)w3_frag; p.b3 = b3; p.y = (bf16_t*)y;
    p.M = (long long)B * H * W;
    p.H = H; p.W = W; p.S = S; p.E1 = E1; p.E3 = E3; p.row_b = 2 * S + 16; p.n_slots = 0;
    MV_CHECK_ARG(p.M < (1ll << 31) - 8192, "mv_fire_expand_fwd: %lld pixels", p.M);
    hipStream_t st = (hipStream_t)stream_;
    // 256 pixels per workgroup (every weight fragment feeds two pixel tiles per wave) while that leaves two workgroups per CU
    // busy and resident; flag "fire_expand_m256": at any size (the parity tests run both tiles on small maps)
    const bool wide = (p.M >= 256ll * 512 || get_flag("fire_expand_m256")) && flat_lds_bytes(256, W, S) <= (size_t)FE_LDS_TWO;
    if (wide) {
        set_kernel_name("fire_expand_m256");
        return fire_go_kc<2>(p, st);
    }
    set_kernel_name("fire_expand_m128");
    return fire_go_kc<1>(p, st);
}

}  // extern "C"
