// Dense-prediction support ops, gfx950: bilinear up-sampling of NHWC feature maps
// (`jax.image.resize(x, shape, method="bilinear")` as used by segmentation/_utils.py:52-58 and deeplabv3.py:66-72) and the
// channel concatenation of the ASPP branches (deeplabv3.py:132-136).  Both are pure data movement: HBM-bound, one pass.
#include "common.h"

namespace mv {

// jax.image.resize, "bilinear" (triangle kernel, half-pixel centres): output pixel o samples the input at
// (o + 0.5) * in / out - 0.5; taps that fall outside the image get weight 0 and the rest is renormalised, which for the 2-tap
// linear kernel is the same as clamping the tap index.  Only out >= in (no antialias window): the callers up-sample.
struct Taps {
    int i0, i1;
    float w1;
};
__device__ __forceinline__ Taps taps_for(int o, int in, int out) {
    const float src = (o + 0.5f) * ((float)in / (float)out) - 0.5f;
    const float f = floorf(src);
    int i0 = (int)f, i1 = i0 + 1;
    const float w1 = src - f;
    i0 = i0 < 0 ? 0 : i0;                      // f = -1 (first half pixel): both taps are pixel 0
    i1 = i1 > in - 1 ? in - 1 : i1;            // last half pixel: both taps are pixel in-1
    return {i0, i1, w1};
}

// the interpolation of the four taps: ONE expression for every kernel of this file, so that the label kernel below selects among
// exactly the values the full-resolution kernels write
__device__ __forceinline__ float bilerp(float v00, float v01, float v10, float v11, float wx, float wy) {
    const float top = v00 + (v01 - v00) * wx, bot = v10 + (v11 - v10) * wx;
    return top + (bot - top) * wy;
}

// one thread per output element; NCHW output: x fastest (coalesced stores, the 2x2 source pixels of neighbouring lanes are the
// same cache lines); NHWC output: channel fastest.
template <typename TI, typename TO, bool NCHW>
__global__ __launch_bounds__(256) void resize_bilinear_kernel(const TI* __restrict__ x, TO* __restrict__ y, int B, int h, int w,
                                                              int C, int H, int W) {
    const long long total = (long long)B * C * H * W;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        int b, c, oy, ox;
        long long r = idx;
        if (NCHW) {
            ox = (int)(r % W); r /= W;
            oy = (int)(r % H); r /= H;
            c = (int)(r % C); b = (int)(r / C);
        } else {
            c = (int)(r % C); r /= C;
            ox = (int)(r % W); r /= W;
            oy = (int)(r % H); b = (int)(r / H);
        }
        const Taps ty = taps_for(oy, h, H), tx = taps_for(ox, w, W);
        const TI* base = x + (long long)b * h * w * C + c;
        const float v00 = io<TI>::ld(base + ((long long)ty.i0 * w + tx.i0) * C);
        const float v01 = io<TI>::ld(base + ((long long)ty.i0 * w + tx.i1) * C);
        const float v10 = io<TI>::ld(base + ((long long)ty.i1 * w + tx.i0) * C);
        const float v11 = io<TI>::ld(base + ((long long)ty.i1 * w + tx.i1) * C);
        io<TO>::st(y + idx, bilerp(v00, v01, v10, v11, tx.w1, ty.w1));
    }
}

// NCHW fp32 output, W % 4 == 0: four consecutive x per thread (one 16-byte store; the y taps and the index arithmetic are shared)
template <typename TI>
__global__ __launch_bounds__(256) void resize_bilinear_nchw4_kernel(const TI* __restrict__ x, float* __restrict__ y, int B, int h,
                                                                    int w, int C, int H, int W) {
    const int W4 = W >> 2;
    const long long total = (long long)B * C * H * W4;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        long long r = idx;
        const int x4 = (int)(r % W4); r /= W4;
        const int oy = (int)(r % H); r /= H;
        const int c = (int)(r % C), b = (int)(r / C);
        const Taps ty = taps_for(oy, h, H);
        const TI* r0 = x + ((long long)b * h + ty.i0) * w * C + c;
        const TI* r1 = x + ((long long)b * h + ty.i1) * w * C + c;
        float o[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const Taps tx = taps_for(x4 * 4 + k, w, W);
            const float v00 = io<TI>::ld(r0 + (long long)tx.i0 * C), v01 = io<TI>::ld(r0 + (long long)tx.i1 * C);
            const float v10 = io<TI>::ld(r1 + (long long)tx.i0 * C), v11 = io<TI>::ld(r1 + (long long)tx.i1 * C);
            o[k] = bilerp(v00, v01, v10, v11, tx.w1, ty.w1);
        }
        *(float4*)(y + idx * 4) = make_float4(o[0], o[1], o[2], o[3]);
    }
}

// ---- label map: bilinear up-sampling + argmax over the classes, the logits at the output resolution never leave registers ----
// jnp.argmax: the first maximum; a NaN beats every number and the first NaN stays (nothing compares greater than it)
__device__ __forceinline__ void argmax_step(float v, int c, float& best, int& arg) {
    if (v > best || (v != v && best == best)) {
        best = v;
        arg = c;
    }
}

template <typename TI> struct pix_vec;                  // the 16-byte piece of a pixel's channel vector
template <> struct pix_vec<float> {
    static constexpr int N = 4;
    __device__ static __forceinline__ void ld(const float* p, float* o) {
        const float4 v = *(const float4*)p;
        o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
    }
};
template <> struct pix_vec<bf16_t> {
    static constexpr int N = 8;
    __device__ static __forceinline__ void ld(const bf16_t* p, float* o) {
        const uint4 v = *(const uint4*)p;
        const uint32_t u[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            o[2 * i] = __uint_as_float(u[i] << 16);
            o[2 * i + 1] = __uint_as_float(u[i] & 0xffff0000u);
        }
    }
};

// Four consecutive output x of one row -> the four labels: the first index of the maximum over the classes of the interpolated
// value.  r0 / r1: the two source rows of the output row, tx: the column taps of the four pixels, wy: the row weight.  The
// channels are walked in increasing order; VEC: C is a whole number of 16-byte pieces and x is 16-byte aligned, so every pixel's
// vector is read in 16-byte loads.  ONE body for the label kernel and the confusion-matrix kernel below: what the second counts
// is by construction what the first stores.
template <typename TI, bool VEC>
__device__ __forceinline__ void resize_argmax4(const TI* __restrict__ r0, const TI* __restrict__ r1, const Taps (&tx)[4], float wy,
                                               int C, int (&arg)[4]) {
    float best[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        best[k] = -INFINITY;                         // class 0 stays the answer unless a later class is greater or a NaN
        arg[k] = 0;
    }
    if (VEC) {
        constexpr int N = pix_vec<TI>::N;
        for (int c = 0; c < C; c += N) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float v00[N], v01[N], v10[N], v11[N];
                pix_vec<TI>::ld(r0 + (long long)tx[k].i0 * C + c, v00);
                pix_vec<TI>::ld(r0 + (long long)tx[k].i1 * C + c, v01);
                pix_vec<TI>::ld(r1 + (long long)tx[k].i0 * C + c, v10);
                pix_vec<TI>::ld(r1 + (long long)tx[k].i1 * C + c, v11);
#pragma unroll
                for (int j = 0; j < N; ++j) {
                    const float v = bilerp(v00[j], v01[j], v10[j], v11[j], tx[k].w1, wy);
                    argmax_step(v, c + j, best[k], arg[k]);
                }
            }
        }
    } else {
        for (int c = 0; c < C; ++c) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float v00 = io<TI>::ld(r0 + (long long)tx[k].i0 * C + c), v01 = io<TI>::ld(r0 + (long long)tx[k].i1 * C + c);
                const float v10 = io<TI>::ld(r1 + (long long)tx[k].i0 * C + c), v11 = io<TI>::ld(r1 + (long long)tx[k].i1 * C + c);
                const float v = bilerp(v00, v01, v10, v11, tx[k].w1, wy);
                argmax_step(v, c, best[k], arg[k]);
            }
        }
    }
}

// A lane owns four consecutive output x of one row (lanes of a wave: consecutive groups, so the label stores of a wave are one
// contiguous 256-byte run and the source pixels it reads are a few neighbouring cache lines of a map that lives in L2).
// Columns past W (ragged last group) are computed at W - 1 and not stored.
template <typename TI, bool VEC>
__global__ __launch_bounds__(256) void resize_argmax_kernel(const TI* __restrict__ x, uint8_t* __restrict__ labels, int B, int h,
                                                            int w, int C, int H, int W) {
    const int W4 = (W + 3) >> 2;
    const long long total = (long long)B * H * W4;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        long long r = idx;
        const int x4 = (int)(r % W4); r /= W4;
        const int oy = (int)(r % H);
        const int b = (int)(r / H);
        const Taps ty = taps_for(oy, h, H);
        const TI* r0 = x + ((long long)b * h + ty.i0) * w * C;
        const TI* r1 = x + ((long long)b * h + ty.i1) * w * C;
        Taps tx[4];
        int arg[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int ox = x4 * 4 + k;
            tx[k] = taps_for(ox < W ? ox : W - 1, w, W);
        }
        resize_argmax4<TI, VEC>(r0, r1, tx, ty.w1, C, arg);
        uint8_t* out = labels + ((long long)b * H + oy) * W + (long long)x4 * 4;
        if (x4 * 4 + 4 <= W && ((uintptr_t)out & 3) == 0) {
            *(uint32_t*)out = (uint32_t)arg[0] | ((uint32_t)arg[1] << 8) | ((uint32_t)arg[2] << 16) | ((uint32_t)arg[3] << 24);
        } else {                                     // ragged W % 4 tail, or rows that do not start on a 4-byte boundary
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (x4 * 4 + k < W) out[k] = (uint8_t)arg[k];
        }
    }
}

// ---- confusion matrix: mat[target][prediction] += 1 for every pixel whose target is a class ------------------------------------
// Counting is exact integer work, so atomics are deterministic in value.  Real label maps are large uniform regions: the 256
// pixels of a wave usually fall into ONE bin.  So equal bins are combined on chip before anything is added: (1) a lane merges its
// four pixels into at most four (bin, count) slots, usually one; (2) per slot, the wave takes the bin of its first lane that still
// holds one, counts everybody who holds the same (three ballots: the counts are 1 .. 4), and ONE lane adds the sum -- at most
// CONF_ROUNDS times, whoever is left then adds for itself; (3) the adds go to 32-bit counters in LDS where C * C of them fit
// (CONF_LDS_BYTES: C <= 64), flushed once per block -- non-zero counters only -- into the 64-bit matrix; above that straight into the
// matrix, with a wave-wide run (bin, count) kept in registers across the loop so that a uniform region costs a wave one global
// atomic, not one per 256 pixels.
constexpr int CONF_ROUNDS = 4;
constexpr int CONF_LDS_BYTES = 16384;           // the default boundary: C <= 64 counts in LDS (measured)
constexpr int CONF_LDS_MAX_BYTES = 65536;       // what a forced placement may take ("confusion_mode"): C <= 128, or 4 x (C <= 64)
constexpr int CONF_FLUSH_ITERS = 1 << 20;       // 2^20 iterations x 1024 pixels of a block = 2^30 < 2^32: an LDS counter cannot wrap

template <typename T> struct lab4;              // four consecutive labels -> int; elements at or behind `n` read as -1 (not counted)
template <> struct lab4<uint8_t> {
    __device__ static __forceinline__ void ld(const uint8_t* p, long long i, long long n, int (&o)[4]) {
        if (i + 4 <= n && ((uintptr_t)(p + i) & 3) == 0) {
            const uint32_t v = *(const uint32_t*)(p + i);
#pragma unroll
            for (int k = 0; k < 4; ++k) o[k] = (int)((v >> (8 * k)) & 0xffu);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) o[k] = i + k < n ? (int)p[i + k] : -1;
        }
    }
};
template <> struct lab4<int> {
    __device__ static __forceinline__ void ld(const int* p, long long i, long long n, int (&o)[4]) {
        if (i + 4 <= n && ((uintptr_t)(p + i) & 15) == 0) {
            const int4 v = *(const int4*)(p + i);
            o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) o[k] = i + k < n ? p[i + k] : -1;
        }
    }
};

// front end 1: the prediction is the label mv_resize_argmax_nhwc_fwd would have written; neither it nor the logits are stored
template <typename TI, bool VEC, typename LT> struct LogitsFront {
    const TI* x;
    const LT* labels;
    int B, h, w, C, H, W;
    __device__ __forceinline__ long long total() const { return (long long)B * H * ((W + 3) >> 2); }
    __device__ __forceinline__ void load(long long idx, int (&target)[4], int (&pred)[4]) const {
        const int W4 = (W + 3) >> 2;
        long long r = idx;
        const int x4 = (int)(r % W4); r /= W4;
        const int oy = (int)(r % H);
        const int b = (int)(r / H);
        const Taps ty = taps_for(oy, h, H);
        Taps tx[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int ox = x4 * 4 + k;
            tx[k] = taps_for(ox < W ? ox : W - 1, w, W);
        }
        resize_argmax4<TI, VEC>(x + ((long long)b * h + ty.i0) * w * C, x + ((long long)b * h + ty.i1) * w * C, tx, ty.w1, C, pred);
        const long long row = ((long long)b * H + oy) * W;
        lab4<LT>::ld(labels, row + (long long)x4 * 4, row + W, target);          // columns past W: -1
    }
};

// front end 2: two label maps
template <typename PT, typename LT> struct LabelsFront {
    const PT* pred;
    const LT* labels;
    long long n;
    __device__ __forceinline__ long long total() const { return (n + 3) >> 2; }
    __device__ __forceinline__ void load(long long idx, int (&target)[4], int (&p)[4]) const {
        lab4<LT>::ld(labels, idx * 4, n, target);
        lab4<PT>::ld(pred, idx * 4, n, p);
    }
};

template <typename Front, bool LDS>
__global__ __launch_bounds__(256) void confusion_kernel(const Front f, unsigned long long* __restrict__ mat, int C, int copies,
                                                        int flush_iters) {
    extern __shared__ uint32_t conf_hist[];         // LDS: copies x C x C counters (copies = 4: one histogram per wave)
    const int tid = threadIdx.x, lane = tid & 63, cells = C * C;
    uint32_t* hist = conf_hist + (copies > 1 ? (tid >> 6) * cells : 0);
    if (LDS) {
        for (int i = tid; i < cells * copies; i += 256) conf_hist[i] = 0;
        __syncthreads();
    }
    int run_bin = -1;                               // !LDS: the wave's pending adds to one bin (wave-uniform)
    unsigned long long run_n = 0;
    const long long total = f.total();
    int iters = 0;
    // block-uniform trip count: every lane of the block stays in the loop (ballots, barriers), lanes past the end hold no bins
    for (long long base = (long long)blockIdx.x * 256; base < total; base += (long long)gridDim.x * 256) {
        int bin[4], cnt[4];
        {
            int target[4] = {-1, -1, -1, -1}, pred[4] = {0, 0, 0, 0};
            if (base + tid < total) f.load(base + tid, target, pred);
#pragma unroll
            for (int k = 0; k < 4; ++k) {           // a pixel counts iff 0 <= target < C (255, any other value >= C, negatives: not)
                const bool ok = (unsigned)target[k] < (unsigned)C && (unsigned)pred[k] < (unsigned)C;
                bin[k] = ok ? (ok ? target[k] : 0) * C + pred[k] : -1;      // (no product is formed from a target out of range)
                cnt[k] = ok ? 1 : 0;
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k)                 // (1) the lane's own pixels: later equal bins fold into the first
#pragma unroll
            for (int j = k + 1; j < 4; ++j)
                if (bin[j] >= 0 && bin[j] == bin[k]) {
                    cnt[k] += cnt[j];
                    bin[j] = -1;
                }
#pragma unroll
        for (int k = 0; k < 4; ++k) {               // (2) across the wave, slot by slot (slots 1 .. 3 are usually empty everywhere)
            int mine = bin[k];
            unsigned long long active = __ballot(mine >= 0);
            for (int round = 0; active != 0 && round < CONF_ROUNDS; ++round) {
                const int lead = __ffsll((long long)active) - 1;
                const int b = __builtin_amdgcn_readlane(mine, lead);          // lead comes from a ballot: wave-uniform
                const bool same = mine == b;
                const unsigned long long who = __ballot(same);
                const uint32_t sum = (uint32_t)__popcll(__ballot(same && (cnt[k] & 1))) + 2u * (uint32_t)__popcll(__ballot(same && (cnt[k] & 2))) +
                                     4u * (uint32_t)__popcll(__ballot(same && (cnt[k] & 4)));
                if (LDS) {
                    if (lane == lead) atomicAdd(&hist[b], sum);
                } else if (round == 0 && b == run_bin) {
                    run_n += sum;
                } else if (round == 0) {
                    if (lane == 0 && run_n) atomicAdd(&mat[run_bin], run_n);
                    run_bin = b;
                    run_n = sum;
                } else {
                    if (lane == lead) atomicAdd(&mat[b], (unsigned long long)sum);
                }
                if (same) mine = -1;
                active &= ~who;
            }
            if (mine >= 0) {                        // more than CONF_ROUNDS different bins in the wave: everybody left adds alone
                if (LDS) atomicAdd(&hist[mine], (uint32_t)cnt[k]);
                else atomicAdd(&mat[mine], (unsigned long long)cnt[k]);
            }
        }
        if (LDS && ++iters == flush_iters) {        // before 32 bits can wrap: flush and start again (block-uniform)
            iters = 0;
            __syncthreads();
            for (int i = tid; i < cells; i += 256) {
                unsigned long long v = 0;
                for (int q = 0; q < copies; ++q) {
                    v += conf_hist[q * cells + i];
                    conf_hist[q * cells + i] = 0;
                }
                if (v) atomicAdd(&mat[i], v);
            }
            __syncthreads();
        }
    }
    if (LDS) {                                      // (3) once per block, the counters that were touched
        __syncthreads();
        for (int i = tid; i < cells; i += 256) {
            unsigned long long v = 0;
            for (int q = 0; q < copies; ++q) v += conf_hist[q * cells + i];
            if (v) atomicAdd(&mat[i], v);
        }
    } else if (lane == 0 && run_n) {
        atomicAdd(&mat[run_bin], run_n);
    }
}

// rows x row_bytes strided copy in 16-byte (or, for odd sizes, 2-byte) pieces
template <typename T>
__global__ __launch_bounds__(256) void copy_rows_kernel(const char* __restrict__ src, char* __restrict__ dst, long long rows,
                                                        int pieces, long long src_pitch, long long dst_pitch) {
    const long long total = rows * pieces;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        const long long r = idx / pieces;
        const int p = (int)(idx - r * pieces);
        *(T*)(dst + r * dst_pitch + (long long)p * sizeof(T)) = *(const T*)(src + r * src_pitch + (long long)p * sizeof(T));
    }
}

static int grid_of(long long n) {
    long long g = (n + 255) / 256;
    return (int)(g > 256 * 16 ? 256 * 16 : (g < 1 ? 1 : g));
}

// where the counters of a C-class matrix live: 0 = global, else the number of LDS histograms per block (1, or 4 = one per wave).
// "confusion_mode" (tests, tools/time_metrics.py): 1 = global, 2 = one LDS histogram, 3 = one per wave where four fit.
static int confusion_copies(int C) {
    const int mode = get_flag("confusion_mode");
    const size_t bytes = (size_t)C * C * sizeof(uint32_t);
    if (mode == 1 || bytes > (size_t)(mode ? CONF_LDS_MAX_BYTES : CONF_LDS_BYTES)) return 0;
    return mode == 3 && 4 * bytes <= (size_t)CONF_LDS_MAX_BYTES ? 4 : 1;
}

template <typename Front>
static void launch_confusion(const Front& f, long long lanes, unsigned long long* mat, int C, const char* name, hipStream_t st) {
    const int copies = confusion_copies(C);
    const int flush = get_flag("confusion_flush_iters") > 0 ? get_flag("confusion_flush_iters") : CONF_FLUSH_ITERS;
    int grid = grid_of(lanes);
    set_kernel_name(name);
    if (copies) {
        grid = grid > 2048 ? 2048 : grid;            // a block flushes up to C * C counters: fewer, longer-running blocks
        append_kernel_name(copies > 1 ? "_lds4" : "_lds");
        hipLaunchKernelGGL((confusion_kernel<Front, true>), dim3(grid), dim3(256), (size_t)copies * C * C * sizeof(uint32_t), st, f, mat,
                           C, copies, flush);
    } else {
        append_kernel_name("_global");
        hipLaunchKernelGGL((confusion_kernel<Front, false>), dim3(grid), dim3(256), 0, st, f, mat, C, 1, flush);
    }
}

}  // namespace mv

using namespace mv;

extern "C" {

int mv_resize_bilinear_nhwc_fwd(const void* x, void* y, int N, int h, int w, int C, int H, int W, int in_dtype, int out_dtype,
                                int out_nchw, mv_stream_t stream) {
    MV_CHECK_ARG(x && y && N > 0 && h > 0 && w > 0 && C > 0 && H > 0 && W > 0, "resize_bilinear: bad args");
    if (H < h || W < w) {
        set_error("resize_bilinear: down-sampling (%dx%d -> %dx%d) needs the antialiasing window of jax.image.resize; "
                  "only up-sampling is on the path (segmentation/_utils.py:52-58)", h, w, H, W);
        return MV_E_UNSUPPORTED;
    }
    hipStream_t st = (hipStream_t)stream;
    const long long total = (long long)N * C * H * W;
    set_kernel_name(out_nchw ? "resize_bilinear_nhwc_to_nchw" : "resize_bilinear_nhwc");
    if (out_nchw && out_dtype == MV_F32 && W % 4 == 0 && ((uintptr_t)y % 16 == 0)) {
        if (in_dtype == MV_BF16)
            hipLaunchKernelGGL((resize_bilinear_nchw4_kernel<bf16_t>), dim3(grid_of(total / 4)), dim3(256), 0, st, (const bf16_t*)x,
                               (float*)y, N, h, w, C, H, W);
        else
            hipLaunchKernelGGL((resize_bilinear_nchw4_kernel<float>), dim3(grid_of(total / 4)), dim3(256), 0, st, (const float*)x,
                               (float*)y, N, h, w, C, H, W);
        MV_LAUNCH_CHECK();
        return MV_OK;
    }
#define GO(TI, TO)                                                                                                        \
    do {                                                                                                                  \
        if (out_nchw)                                                                                                     \
            hipLaunchKernelGGL((resize_bilinear_kernel<TI, TO, true>), dim3(grid_of(total)), dim3(256), 0, st, (const TI*)x, \
                               (TO*)y, N, h, w, C, H, W);                                                                 \
        else                                                                                                              \
            hipLaunchKernelGGL((resize_bilinear_kernel<TI, TO, false>), dim3(grid_of(total)), dim3(256), 0, st, (const TI*)x, \
                               (TO*)y, N, h, w, C, H, W);                                                                 \
    } while (0)
    if (in_dtype == MV_BF16 && out_dtype == MV_F32) GO(bf16_t, float);
    else if (in_dtype == MV_BF16) GO(bf16_t, bf16_t);
    else if (out_dtype == MV_F32) GO(float, float);
    else GO(float, bf16_t);
#undef GO
    MV_LAUNCH_CHECK();
    return MV_OK;
}

int mv_resize_argmax_nhwc_fwd(const void* x, void* labels, int B, int h, int w, int C, int H, int W, int x_dtype,
                              mv_stream_t stream) {
    MV_CHECK_ARG(x && labels, "resize_argmax: NULL buffer");
    MV_CHECK_ARG(B > 0 && h > 0 && w > 0 && C > 0 && H > 0 && W > 0, "resize_argmax: bad dimensions B=%d %dx%dx%d -> %dx%d", B, h, w, C,
                 H, W);
    MV_CHECK_ARG(C <= 256, "resize_argmax: %d classes do not fit a uint8 label (at most 256)", C);
    MV_CHECK_ARG(x_dtype == MV_F32 || x_dtype == MV_BF16, "resize_argmax: bad dtype %d", x_dtype);
    MV_CHECK_ARG(H >= h && W >= w, "resize_argmax: down-sampling (%dx%d -> %dx%d) is not supported, only up-sampling", h, w, H, W);
    hipStream_t st = (hipStream_t)stream;
    const int grid = grid_of((long long)B * H * ((W + 3) / 4));
    const bool vec = (uintptr_t)x % 16 == 0 && C % (x_dtype == MV_BF16 ? 8 : 4) == 0;
    set_kernel_name(vec ? "resize_argmax_nhwc_v16" : "resize_argmax_nhwc");
#define GO(TI, V) \
    hipLaunchKernelGGL((resize_argmax_kernel<TI, V>), dim3(grid), dim3(256), 0, st, (const TI*)x, (uint8_t*)labels, B, h, w, C, H, W)
    if (x_dtype == MV_BF16) {
        if (vec) GO(bf16_t, true);
        else GO(bf16_t, false);
    } else {
        if (vec) GO(float, true);
        else GO(float, false);
    }
#undef GO
    MV_LAUNCH_CHECK();
    return MV_OK;
}

int mv_confusion_from_logits(const void* logits, const void* labels, unsigned long long* mat, int B, int h, int w, int C, int H,
                             int W, int logits_dtype, int label_bytes, mv_stream_t stream) {
    MV_CHECK_ARG(logits && labels && mat, "confusion_from_logits: NULL buffer");
    MV_CHECK_ARG(B > 0 && h > 0 && w > 0 && H > 0 && W > 0, "confusion_from_logits: bad dimensions B=%d %dx%d -> %dx%d", B, h, w, H, W);
    MV_CHECK_ARG(C >= 1 && C <= 256, "confusion_from_logits: %d classes (1 .. 256)", C);
    MV_CHECK_ARG(logits_dtype == MV_F32 || logits_dtype == MV_BF16, "confusion_from_logits: bad dtype %d", logits_dtype);
    MV_CHECK_ARG(label_bytes == 1 || label_bytes == 4, "confusion_from_logits: labels are uint8 or int32, not %d bytes wide", label_bytes);
    MV_CHECK_ARG(H >= h && W >= w, "confusion_from_logits: down-sampling (%dx%d -> %dx%d) is not supported, only up-sampling", h, w, H, W);
    MV_CHECK_ARG(label_bytes == 1 || (uintptr_t)labels % 4 == 0, "confusion_from_logits: int32 labels must be 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const long long lanes = (long long)B * H * ((W + 3) / 4);
    const bool vec = (uintptr_t)logits % 16 == 0 && C % (logits_dtype == MV_BF16 ? 8 : 4) == 0;
    const char* name = vec ? "resize_argmax_confusion_v16" : "resize_argmax_confusion";
#define GO(TI, V, LT)                                                                                  \
    do {                                                                                               \
        const LogitsFront<TI, V, LT> f{(const TI*)logits, (const LT*)labels, B, h, w, C, H, W};         \
        launch_confusion(f, lanes, mat, C, name, st);                                                  \
    } while (0)
#define GO_L(TI, V)                           \
    do {                                      \
        if (label_bytes == 1) GO(TI, V, uint8_t); \
        else GO(TI, V, int);                  \
    } while (0)
    if (logits_dtype == MV_BF16) {
        if (vec) GO_L(bf16_t, true);
        else GO_L(bf16_t, false);
    } else {
        if (vec) GO_L(float, true);
        else GO_L(float, false);
    }
#undef GO_L
#undef GO
    MV_LAUNCH_CHECK();
    return MV_OK;
}

int mv_confusion_from_labels(const void* pred, const void* labels, unsigned long long* mat, long long n, int C, int pred_bytes,
                             int label_bytes, mv_stream_t stream) {
    MV_CHECK_ARG(pred && labels && mat, "confusion_from_labels: NULL buffer");
    MV_CHECK_ARG(n > 0, "confusion_from_labels: bad size n=%lld", n);
    MV_CHECK_ARG(C >= 1 && C <= 256, "confusion_from_labels: %d classes (1 .. 256)", C);
    MV_CHECK_ARG((pred_bytes == 1 || pred_bytes == 4) && (label_bytes == 1 || label_bytes == 4),
                 "confusion_from_labels: label maps are uint8 or int32, not %d / %d bytes wide", pred_bytes, label_bytes);
    MV_CHECK_ARG((pred_bytes == 1 || (uintptr_t)pred % 4 == 0) && (label_bytes == 1 || (uintptr_t)labels % 4 == 0),
                 "confusion_from_labels: int32 label maps must be 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const long long lanes = (n + 3) / 4;
#define GO(PT, LT)                                                                 \
    do {                                                                           \
        const LabelsFront<PT, LT> f{(const PT*)pred, (const LT*)labels, n};        \
        launch_confusion(f, lanes, mat, C, "label_confusion", st);                 \
    } while (0)
    if (pred_bytes == 1) {
        if (label_bytes == 1) GO(uint8_t, uint8_t);
        else GO(uint8_t, int);
    } else {
        if (label_bytes == 1) GO(int, uint8_t);
        else GO(int, int);
    }
#undef GO
    MV_LAUNCH_CHECK();
    return MV_OK;
}

int mv_copy_rows(const void* src, void* dst, int64_t rows, int64_t row_bytes, int64_t src_pitch, int64_t dst_pitch,
                 mv_stream_t stream) {
    MV_CHECK_ARG(src && dst && rows > 0 && row_bytes > 0 && src_pitch >= row_bytes && dst_pitch >= row_bytes, "copy_rows: bad args");
    MV_CHECK_ARG(row_bytes % 2 == 0 && src_pitch % 2 == 0 && dst_pitch % 2 == 0, "copy_rows: sizes must be multiples of 2 bytes");
    hipStream_t st = (hipStream_t)stream;
    set_kernel_name("copy_rows");
    const bool v16 = row_bytes % 16 == 0 && src_pitch % 16 == 0 && dst_pitch % 16 == 0 && ((uintptr_t)src % 16 == 0) &&
                     ((uintptr_t)dst % 16 == 0);
    if (v16) {
        const int pieces = (int)(row_bytes / 16);
        hipLaunchKernelGGL((copy_rows_kernel<uint4>), dim3(grid_of(rows * pieces)), dim3(256), 0, st, (const char*)src, (char*)dst,
                           (long long)rows, pieces, (long long)src_pitch, (long long)dst_pitch);
    } else {
        const int pieces = (int)(row_bytes / 2);
        hipLaunchKernelGGL((copy_rows_kernel<uint16_t>), dim3(grid_of(rows * pieces)), dim3(256), 0, st, (const char*)src,
                           (char*)dst, (long long)rows, pieces, (long long)src_pitch, (long long)dst_pitch);
    }
    MV_LAUNCH_CHECK();
    return MV_OK;
}

}  // extern "C"
