// Shared device/host helpers for the gfx950 kernels.  CDNA4 only: wave = 64 lanes.
#pragma once
#include <atomic>
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/eqxvision_amd.h"
#include "route.h"

namespace mv {

typedef uint16_t bf16_t;  // raw bf16 bits

__device__ __forceinline__ float bf2f(bf16_t v) { return __uint_as_float(((uint32_t)v) << 16); }

// round-to-nearest-even fp32 -> bf16: plain casts, which hipcc lowers to the gfx950 hardware converter
// (v_cvt_pk_bf16_f32, two values per instruction) instead of ~6 VALU ops of bit arithmetic per value
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ bf16_t f2bf(float f) { return __builtin_bit_cast(bf16_t, (__bf16)f); }
// fl(fl(a x) + fl(b y)): two rounded products and one rounded sum, never contracted into an fma (what float32 numpy computes for
// a * x + b * y).  hipcc's __fmul_rn / __fadd_rn are plain * and + and fuse under the default -ffp-contract=fast.
__device__ __forceinline__ float mul_add_rn(float a, float x, float b, float y) {
#pragma clang fp contract(off)
    const float p = a * x, q = b * y;
    return p + q;
}
__device__ __forceinline__ uint32_t pack_bf2(float lo, float hi) {
    bf16x2_t v;
    v[0] = (__bf16)lo;
    v[1] = (__bf16)hi;
    return __builtin_bit_cast(uint32_t, v);
}

template <typename T> struct io;
template <> struct io<float> {
    __device__ static __forceinline__ float ld(const float* p) { return *p; }
    __device__ static __forceinline__ void st(float* p, float v) { *p = v; }
};
template <> struct io<bf16_t> {
    __device__ static __forceinline__ float ld(const bf16_t* p) { return bf2f(*p); }
    __device__ static __forceinline__ void st(bf16_t* p, float v) { *p = f2bf(v); }
};

__device__ __forceinline__ float gelu_tanh_f(float x) {
    // jax.nn.gelu(approximate=True): 0.5x(1+tanh(u)), u = sqrt(2/pi)(x+0.044715x^3)
    // 0.5(1+tanh(u)) = 1/(1+exp(-2u)), exp(-2u) = exp2(x*(k0 + k1*x^2)): one v_exp_f32 + one v_rcp_f32 (hardware
    // approximations, ~1 ulp) and four plain VALU ops; no IEEE division, no clamp (exp2 -> +inf gives rcp -> 0 -> -0, the
    // limit for very negative x; exp2 -> 0 gives x).  The epilogue of the 768->3072 fc1 GEMM spent ~28% of the layer in the
    // first version of this function, and the fused Swin MLP kernel (ln_mlp.hip) is bound by it.
    const float k0 = -2.0f * 0.7978845608028654f * 1.4426950408889634f;  // -2*sqrt(2/pi)*log2(e)
    const float k1 = k0 * 0.044715f;
    const float t = x * fmaf(k1, x * x, k0);
    return x * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(t));
}

// Two activations at once on the packed-fp32 VALU ops (v_pk_mul_f32 / v_pk_fma_f32 / v_pk_add_f32 take two values per
// lane per issue slot); the two transcendentals per value stay scalar.  Returns the bf16 pair.
typedef float f32x2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t gelu_tanh_pack2(float a, float b) {
    const float k0 = -2.0f * 0.7978845608028654f * 1.4426950408889634f;
    const float k1 = k0 * 0.044715f;
    f32x2_t x = {a, b};
    const f32x2_t kk0 = {k0, k0}, kk1 = {k1, k1}, one = {1.0f, 1.0f};
    f32x2_t t = x * __builtin_elementwise_fma(kk1, x * x, kk0);
    f32x2_t e = {__builtin_amdgcn_exp2f(t[0]), __builtin_amdgcn_exp2f(t[1])};
    e = e + one;
    f32x2_t r = {__builtin_amdgcn_rcpf(e[0]), __builtin_amdgcn_rcpf(e[1])};
    x = x * r;
    return pack_bf2(x[0], x[1]);
}

template <int ACT> __device__ __forceinline__ float apply_act(float v) {
    if (ACT == MV_ACT_RELU) return v > 0.f ? v : 0.f;
    if (ACT == MV_ACT_GELU_TANH) return gelu_tanh_f(v);
    return v;
}
__device__ __forceinline__ float apply_act_rt(float v, int act) {
    if (act == MV_ACT_RELU) return v > 0.f ? v : 0.f;
    if (act == MV_ACT_GELU_TANH) return gelu_tanh_f(v);
    if (act == MV_ACT_HARD_SWISH) return v * fminf(fmaxf(v + 3.0f, 0.f), 6.0f) * (1.0f / 6.0f);       // jax.nn.hard_swish
    if (act == MV_ACT_HARD_SIGMOID) return fminf(fmaxf(v + 3.0f, 0.f), 6.0f) * (1.0f / 6.0f);         // jax.nn.hard_sigmoid
    if (act == MV_ACT_SIGMOID) return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.4426950408889634f * v));
    if (act == MV_ACT_SILU) return v * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.4426950408889634f * v));
    return v;
}

// reductions over the 64 lanes of a wave (every lane gets the result)
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// ---- host side ------------------------------------------------------------------------
void set_error(const char* fmt, ...);
void set_kernel_name(const char* name);
void append_kernel_name(const char* suffix);
int get_flag(const char* name);
// the scratch the host handed over with mv_set_scratch for the next launch on `stream`: returned (and forgotten) if it holds
// at least `need` bytes, else nullptr
void* take_scratch(hipStream_t stream, size_t need);            // (SCRATCH_SYNC_BYTES, the head of every offer: route.h)
void* peek_scratch(hipStream_t stream, size_t* bytes);
// the partial sums of a split reduction, `part_elems` floats each, from that offer: min(want, what fits) parts if that is at least
// `least`, else 0 and *part = nullptr (the offer stays on offer).  runtime.hip says where in the offer they lie and why.
long long take_scratch_parts(hipStream_t stream, long long want, long long least, long long part_elems, float** part);
// out[i] = part[0][i] + part[1][i] + ... + part[parts - 1][i] in index order, for i < n (train_bwd.hip)
void sum_parts(hipStream_t stream, const float* part, float* out, long long n, int parts);
size_t splitk_scratch_bytes(long long M, long long N, long long kred);       // igemm8.hip
const void* zero_page(hipStream_t stream);  // >= 4 KiB of device zeros for the current device

inline size_t dsize(int dt) { return dt == MV_BF16 ? 2 : 4; }

#define MV_CHECK_ARG(cond, ...)                      \
    do {                                             \
        if (!(cond)) {                               \
            mv::set_error(__VA_ARGS__);              \
            return MV_E_INVALID;                     \
        }                                            \
    } while (0)

// the matrix-core epilogues implement none / relu / gelu only
#define MV_CHECK_FUSED_ACT(act, who) \
    MV_CHECK_ARG((act) >= MV_ACT_NONE && (act) <= MV_ACT_GELU_TANH, who ": activation %d is not fused into this entry (use mv_eltwise_fwd)", (act))

#define MV_LAUNCH_CHECK()                                                            \
    do {                                                                             \
        hipError_t e__ = hipGetLastError();                                          \
        if (e__ != hipSuccess) {                                                     \
            mv::set_error("%s:%d launch failed: %s", __FILE__, __LINE__, hipGetErrorString(e__)); \
            return (int)e__;                                                         \
        }                                                                            \
    } while (0)

// hipFuncAttributeMaxDynamicSharedMemorySize is a PER-DEVICE property of a kernel: a launch site keeps one of these (static) and asks
// before every launch; the attribute is set the first time the site launches on a device (and again if it needs more LDS than any
// earlier launch asked for on that device).  Lock-free: two threads racing on the first launch both set the same value.
struct LdsAttrSite {
    std::atomic<int> bytes[16];                 // per device ordinal (mod 16): the largest size already granted
    LdsAttrSite() { for (auto& b : bytes) b.store(0, std::memory_order_relaxed); }
    hipError_t ensure(const void* kern, size_t need) {
        int dev = 0;
        hipError_t e = hipGetDevice(&dev);
        if (e != hipSuccess) return e;
        std::atomic<int>& b = bytes[dev & 15];
        if (b.load(std::memory_order_acquire) >= (int)need) return hipSuccess;
        e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)need);
        if (e == hipSuccess) b.store((int)need, std::memory_order_release);
        return e;
    }
};

#define MV_HIP(call)                                                                 \
    do {                                                                             \
        hipError_t e__ = (call);                                                     \
        if (e__ != hipSuccess) {                                                     \
            (void)hipGetLastError(); /* clear the sticky error so later launches are not blamed */ \
            mv::set_error("%s:%d %s: %s", __FILE__, __LINE__, #call, hipGetErrorString(e__)); \
            return (int)e__;                                                         \
        }                                                                            \
    } while (0)

// The convolution geometry of the igemm parameter structs (IgemmP, Igemm2P): Ho, Wo, M, strides, pads, dilations, the zero page
// that out-of-image taps read, and the 31-bit range checks (pixel_index32: the kernel indexes INPUT pixels with 32 bits too).
template <class P> int fill_geometry(P& p, const ConvShape& s, const char* who, bool pixel_index32, hipStream_t st) {
    p.zero = (const bf16_t*)zero_page(st);
    if (!p.zero) {
        set_error("%s: zero page allocation failed", who);
        return MV_E_OOM;
    }
    if (pixel_index32 && (long long)s.N * s.H * s.W >= (1LL << 31) - (1LL << 20)) {
        set_error("%s: %lld input pixels do not fit the 32-bit pixel index", who, (long long)s.N * s.H * s.W);
        return MV_E_UNSUPPORTED;
    }
    p.N = s.N; p.H = s.H; p.W = s.W; p.C = s.C; p.K = s.K; p.R = s.R; p.S = s.S;
    p.Ho = s.Ho(); p.Wo = s.Wo();
    p.sh = s.sh; p.sw = s.sw; p.ph = s.ph; p.pw = s.pw; p.dh = s.dh; p.dw = s.dw;
    const long long M = s.M();
    if (M >= (1LL << 31) - 256) {
        set_error("%s: M=%lld too large", who, M);
        return MV_E_UNSUPPORTED;
    }
    p.M = (int)M;
    p.act = s.act;
    return MV_OK;
}

// Launch grids of the grid-stride kernels: one thread per element, capped at 16 blocks per CU
inline int grid_for(long long n, int block = 256) {
    long long g = (n + block - 1) / block;
    if (g > 256 * 16) g = 256 * 16;
    if (g < 1) g = 1;
    return (int)g;
}

// One (in, out) dtype ladder for the memory-bound entries: dispatch_io calls f(TI{}, TO{}) with the element types of the two
// dtypes (a generic lambda that launches its kernel and returns a status); a dtype outside {MV_F32, MV_BF16} is an error that
// names the entry, raised before any HIP call.  dispatch_dtype is the same for entries with one dtype.
template <class F> int dispatch_dtype(const char* who, int dtype, F&& f) {
    if (dtype == MV_BF16) return f(bf16_t{});
    if (dtype == MV_F32) return f(float{});
    set_error("%s: unknown dtype %d", who, dtype);
    return MV_E_INVALID;
}
template <class F> int dispatch_io(const char* who, int in_dtype, int out_dtype, F&& f) {
    return dispatch_dtype(who, in_dtype, [&](auto ti) { return dispatch_dtype(who, out_dtype, [&](auto to) { return f(ti, to); }); });
}

// Launchers with a caller in ANOTHER translation unit than the one that defines them (route.h holds the rule that picks among
// them, its predicates and the kernels' names).  A launcher only its own file's entries call is static there; the ones only the
// routing entries of conv_fallback.hip call are declared in conv_launchers.h.
int stream1x1_launch(const void* x, const void* w, const float* scale, const float* shift, const void* residual,
                     void* y, long long M, int C, int K, int act, int out_dtype, hipStream_t stream);
int igemm2_launch(const void* x, const void* w, const float* scale, const float* shift, const void* residual, void* y,
                  const ConvShape& s, int tile, int tok, hipStream_t stream);   // tile: 1 = 256x64, 2 = 256x128, 3 = 256x256, 0 = its own rule
int device_status(int clear, unsigned* out);              // igemm8.hip: the status word of mv_device_status
unsigned* device_status_word();                           // its device address (nullptr if the runtime cannot give it)
int igemm8_launch(const void* x, const void* w, const float* scale, const float* shift, const void* residual, void* y,
                  const ConvShape& s, int tok, int tile, hipStream_t st);       // tile: 1 = 256x256, 2 = 128x256, 3 = 256x128
int swin_mfma_supported(int C, int heads, int ws_h, int ws_w, int dtype);
int swin_mfma_launch(const void* qkv, const float* bias, void* out, int B, int Hf, int Wf, int C, int heads, int ws_h,
                     int ws_w, int shift_h, int shift_w, const uint32_t* drop_keys, float keep, hipStream_t st,
                     const float* rnorm = nullptr, const float* logit_mul = nullptr);   // rnorm given: Swin V2's cosine logits
int conv3x3c64_v2_launch(const void* x, const void* w, const float* scale, const float* shift, void* y, int N, int H,
                         int W, int act, hipStream_t stream);
int skinny_launch(const void* x, const void* w, const float* scale, const float* shift, void* y, long long M, int C, int K,
                  int act, int out_dtype, hipStream_t stream);
int mha_mfma_supported(int N, int dh, int dtype);
int mha_mfma_launch(const void* qkv, int head_major, void* out, float* probs, int B, int N, int H, int dh, float scale,
                    const uint32_t* drop_keys, float keep, hipStream_t st);

}  // namespace mv
