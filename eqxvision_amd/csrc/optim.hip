// Optimisers over a WHOLE parameter set in one launch (include/eqxvision_amd.h: mv_optim_tensor).
// A model has 150+ float leaves, most of them a few hundred elements (BatchNorm / LayerNorm vectors, biases): one launch per leaf
// is 300+ launches per step behind the backward pass.  Here the host keeps ONE record per tensor in a device buffer (as
// preprocess.hip does per image) and a 256-thread workgroup owns one chunk of MV_OPTIM_CHUNK = 4096 elements of one tensor:
//   * its record is found by binary search of first_block over blockIdx.x -- wave-uniform, once, scalar loads;
//   * lane t takes elements [1024 j + 4 t, +4) of the chunk for j = 0..3: one float4 per operand per trip when every pointer of
//     the record is 16-byte aligned (chunks start at multiples of 4096 elements, so alignment is a property of the tensor);
//     the last n % 4 elements, and every element of an unaligned tensor, go one by one through the same code path;
//   * plain vector stores, no atomics; the squared norm is reduced in a fixed order (below), so it has the same bits every run.
// Whatever first_block says, a workgroup only touches elements [0, n) of the record it picked.
// The kernels are HBM streams; bytes moved per element: sgd 8 (16 with momentum: m is read and written), adamw 24 (28 with weight
// decay: the parameter is read), apply 12, ema 12 (4 when it copies), squared norm 4.
#include "common.h"

namespace mv {

namespace {

constexpr int OPT_THREADS = 256;
constexpr int OPT_TRIPS = MV_OPTIM_CHUNK / (4 * OPT_THREADS);
static_assert(OPT_TRIPS * 4 * OPT_THREADS == MV_OPTIM_CHUNK, "a chunk is a whole number of float4 trips");

struct OptChunk {
    mv_optim_tensor r;
    long long base;     // first element of this workgroup's chunk
    int cnt;            // elements of the chunk that exist (<= 0: nothing to do)
    bool vec;           // every pointer of the record is 16-byte aligned
};

__device__ __forceinline__ OptChunk opt_chunk(const mv_optim_tensor* __restrict__ recs, int n_tensors) {
    const long long b = blockIdx.x;
    int lo = 0, hi = n_tensors - 1;
    while (lo < hi) {                                   // the last record with first_block <= b
        const int mid = (lo + hi + 1) >> 1;
        if (recs[mid].first_block <= b) lo = mid; else hi = mid - 1;
    }
    OptChunk c;
    c.r = recs[lo];
    c.base = (b - c.r.first_block) * (long long)MV_OPTIM_CHUNK;
    const long long left = c.r.n - c.base;
    c.cnt = (b < c.r.first_block || left <= 0) ? 0 : (int)(left < MV_OPTIM_CHUNK ? left : MV_OPTIM_CHUNK);
    const uintptr_t bits = (uintptr_t)c.r.grad | (uintptr_t)c.r.param | (uintptr_t)c.r.m | (uintptr_t)c.r.v | (uintptr_t)c.r.out;
    c.vec = (bits & 15) == 0;
    return c;
}

// four elements from p + i of which `rem` exist (rem > 0); the missing ones read as 0
__device__ __forceinline__ float4 ld4(const float* __restrict__ p, long long i, int rem, bool vec) {
    if (vec && rem >= 4) return *reinterpret_cast<const float4*>(p + i);
    float4 r = {0.f, 0.f, 0.f, 0.f};
    r.x = p[i];
    if (rem > 1) r.y = p[i + 1];
    if (rem > 2) r.z = p[i + 2];
    if (rem > 3) r.w = p[i + 3];
    return r;
}

__device__ __forceinline__ void st4(float* __restrict__ p, long long i, int rem, bool vec, float4 v) {
    if (vec && rem >= 4) { *reinterpret_cast<float4*>(p + i) = v; return; }
    p[i] = v.x;
    if (rem > 1) p[i + 1] = v.y;
    if (rem > 2) p[i + 2] = v.z;
    if (rem > 3) p[i + 3] = v.w;
}

// the four waves' sums in wave order through LDS, after a fixed butterfly over each wave; valid in thread 0
__device__ __forceinline__ float block_sum_ordered(float v) {
    __shared__ float part[OPT_THREADS / 64];
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((part[0] + part[1]) + part[2]) + part[3];
}

__global__ __launch_bounds__(OPT_THREADS) void optim_sqnorm_part_kernel(const mv_optim_tensor* __restrict__ recs, int n_tensors,
                                                                         float* __restrict__ partial) {
    const OptChunk c = opt_chunk(recs, n_tensors);
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < OPT_TRIPS; ++j) {
        const int off = j * 4 * OPT_THREADS + 4 * (int)threadIdx.x, rem = c.cnt - off;
        if (rem > 0) {
            const float4 g = ld4(c.r.grad, c.base + off, rem, c.vec);
            acc = fmaf(g.x, g.x, acc);
            acc = fmaf(g.y, g.y, acc);
            acc = fmaf(g.z, g.z, acc);
            acc = fmaf(g.w, g.w, acc);
        }
    }
    const float s = block_sum_ordered(acc);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

__global__ __launch_bounds__(OPT_THREADS) void optim_sqnorm_finish_kernel(const float* __restrict__ partial, long long total_blocks,
                                                                           float* __restrict__ out2, float max_norm) {
    float acc = 0.f;
    for (long long i = threadIdx.x; i < total_blocks; i += OPT_THREADS) acc += partial[i];
    const float s = block_sum_ordered(acc);
    if (threadIdx.x == 0) {
        const float norm = sqrtf(s);
        out2[0] = s;
        out2[1] = norm < max_norm ? 1.f : max_norm / norm;          // optax.clip_by_global_norm
    }
}

struct OptHyper {
    float lr, b1, b2, omb1, omb2, eps, wd, bc1, bc2;
    int nesterov;
};

template <int KIND> __device__ __forceinline__ float opt_rule(float g, float p, float& m, float& v, bool has_m, const OptHyper& h) {
    if (KIND == MV_OPT_APPLY) return p + g;
    if (KIND == MV_OPT_SGD) {
        if (!has_m) return -h.lr * g;
        m = g + h.b1 * m;
        return h.nesterov ? -h.lr * (g + h.b1 * m) : -h.lr * m;
    }
    m = h.b1 * m + h.omb1 * g;
    v = h.b2 * v + h.omb2 * g * g;
    return -h.lr * ((m / h.bc1) / (sqrtf(v / h.bc2) + h.eps) + h.wd * p);
}

// e = fadd(fmul(d, e), fmul(omd, p)): what float32 numpy computes for d * e + omd * p
__device__ __forceinline__ float4 ema4(const float4 e, const float4 p, const OptHyper& h) {
    float4 o;
    o.x = mul_add_rn(h.b1, e.x, h.omb1, p.x);
    o.y = mul_add_rn(h.b1, e.y, h.omb1, p.y);
    o.z = mul_add_rn(h.b1, e.z, h.omb1, p.z);
    o.w = mul_add_rn(h.b1, e.w, h.omb1, p.w);
    return o;
}

template <int KIND> __global__ __launch_bounds__(OPT_THREADS) void optim_step_kernel(const mv_optim_tensor* __restrict__ recs,
                                                                                      int n_tensors, const OptHyper h,
                                                                                      const float* __restrict__ scale) {
    const OptChunk c = opt_chunk(recs, n_tensors);
    const float s = scale ? scale[1] : 1.f;
    const bool has_p = c.r.param != nullptr && KIND != MV_OPT_SGD && KIND != MV_OPT_EMA;
    const bool has_m = c.r.m != nullptr && KIND != MV_OPT_APPLY && KIND != MV_OPT_EMA;
    const bool has_v = c.r.v != nullptr && KIND == MV_OPT_ADAMW;
    if (KIND == MV_OPT_APPLY && !has_p) return;
    if (KIND == MV_OPT_ADAMW && !(has_m && has_v)) return;
    const float4 zero = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < OPT_TRIPS; ++j) {
        const int off = j * 4 * OPT_THREADS + 4 * (int)threadIdx.x, rem = c.cnt - off;
        if (rem <= 0) continue;
        const long long i = c.base + off;
        float4 g = ld4(c.r.grad, i, rem, c.vec);
        if (KIND == MV_OPT_EMA) {                       // out is the average: read, unless this update copies, and written
            const float4 e = h.nesterov ? g : ld4(c.r.out, i, rem, c.vec);
            st4(c.r.out, i, rem, c.vec, h.nesterov ? g : ema4(e, g, h));
            continue;
        }
        const float4 p = has_p ? ld4(c.r.param, i, rem, c.vec) : zero;
        float4 m = has_m ? ld4(c.r.m, i, rem, c.vec) : zero;
        float4 v = has_v ? ld4(c.r.v, i, rem, c.vec) : zero;
        if (KIND != MV_OPT_APPLY) { g.x *= s; g.y *= s; g.z *= s; g.w *= s; }
        float4 o;
        o.x = opt_rule<KIND>(g.x, p.x, m.x, v.x, has_m, h);
        o.y = opt_rule<KIND>(g.y, p.y, m.y, v.y, has_m, h);
        o.z = opt_rule<KIND>(g.z, p.z, m.z, v.z, has_m, h);
        o.w = opt_rule<KIND>(g.w, p.w, m.w, v.w, has_m, h);
        if (has_m) st4(c.r.m, i, rem, c.vec, m);
        if (has_v) st4(c.r.v, i, rem, c.vec, v);
        st4(c.r.out, i, rem, c.vec, o);
    }
}

}  // namespace

}  // namespace mv

using namespace mv;

extern "C" {

int mv_optim_sqnorm_f32(const mv_optim_tensor* recs, int n_tensors, int64_t total_blocks, float* partial, float* out2,
                        float max_norm, mv_stream_t stream) {
    MV_CHECK_ARG(recs && partial && out2 && n_tensors > 0, "optim_sqnorm: bad arguments");
    MV_CHECK_ARG(total_blocks >= n_tensors && total_blocks < (1LL << 31), "optim_sqnorm: %lld blocks for %d tensors",
                 (long long)total_blocks, n_tensors);
    MV_CHECK_ARG(max_norm > 0.f, "optim_sqnorm: max_norm = %g must be positive", (double)max_norm);
    set_kernel_name("optim_sqnorm_f32");
    hipLaunchKernelGGL(optim_sqnorm_part_kernel, dim3((unsigned)total_blocks), dim3(OPT_THREADS), 0, (hipStream_t)stream, recs,
                       n_tensors, partial);
    hipLaunchKernelGGL(optim_sqnorm_finish_kernel, dim3(1), dim3(OPT_THREADS), 0, (hipStream_t)stream, partial,
                       (long long)total_blocks, out2, max_norm);
    MV_LAUNCH_CHECK();
    return MV_OK;
}

int mv_optim_step_f32(const mv_optim_tensor* recs, int n_tensors, int64_t total_blocks, int kind, int nesterov, float lr, float b1,
                      float b2, float one_minus_b1, float one_minus_b2, float eps, float weight_decay, float bias_corr1,
                      float bias_corr2, const float* scale, mv_stream_t stream) {
    MV_CHECK_ARG(recs && n_tensors > 0, "optim_step: bad arguments");
    MV_CHECK_ARG(total_blocks >= n_tensors && total_blocks < (1LL << 31), "optim_step: %lld blocks for %d tensors",
                 (long long)total_blocks, n_tensors);
    MV_CHECK_ARG(kind == MV_OPT_SGD || kind == MV_OPT_ADAMW || kind == MV_OPT_APPLY || kind == MV_OPT_EMA, "optim_step: unknown kind %d",
                 kind);
    if (kind == MV_OPT_ADAMW)
        MV_CHECK_ARG(bias_corr1 > 0.f && bias_corr2 > 0.f, "optim_step: adamw needs positive bias corrections (count >= 1)");
    const OptHyper h = {lr, b1, b2, one_minus_b1, one_minus_b2, eps, weight_decay, bias_corr1, bias_corr2, nesterov};
    const dim3 grid((unsigned)total_blocks), block(OPT_THREADS);
    if (kind == MV_OPT_SGD) {
        set_kernel_name("optim_sgd_f32");
        hipLaunchKernelGGL(optim_step_kernel<MV_OPT_SGD>, grid, block, 0, (hipStream_t)stream, recs, n_tensors, h, scale);
    } else if (kind == MV_OPT_ADAMW) {
        set_kernel_name("optim_adamw_f32");
        hipLaunchKernelGGL(optim_step_kernel<MV_OPT_ADAMW>, grid, block, 0, (hipStream_t)stream, recs, n_tensors, h, scale);
    } else if (kind == MV_OPT_EMA) {
        set_kernel_name("optim_ema_f32");
        hipLaunchKernelGGL(optim_step_kernel<MV_OPT_EMA>, grid, block, 0, (hipStream_t)stream, recs, n_tensors, h, scale);
    } else {
        set_kernel_name("optim_apply_f32");
        hipLaunchKernelGGL(optim_step_kernel<MV_OPT_APPLY>, grid, block, 0, (hipStream_t)stream, recs, n_tensors, h, scale);
    }
    MV_LAUNCH_CHECK();
    return MV_OK;
}

}  // extern "C"
