// Classifier tail, gfx950: softmax + top-k of a [B][K] fp32 logit matrix in one launch (jax.nn.softmax + jax.lax.top_k of what
// `vmap(net)` returns).  One workgroup per row; a row is at most 256 KiB and is read k + 1 times, the first time from HBM and
// then from L2 / L1.  No sort, no scratch, no atomics.
#include "common.h"

namespace mv {

constexpr int TOPK_THREADS = 256, TOPK_WAVES = TOPK_THREADS / 64;

// (value, index) as ONE 64-bit key whose unsigned order is "greater value first, then lower index": the high word is the usual
// order-preserving image of the float (-0 counts as +0, so the two zeros tie; every NaN gets the top word and orders above all
// numbers), the low word decreases with the index.  Keys of one row are distinct, so round r selects the largest key below the
// key of round r - 1 and nothing has to be marked as taken.  0 is below every key.
__device__ __forceinline__ unsigned long long topk_key(float v, int i) {
    uint32_t b = __float_as_uint(v == 0.f ? 0.f : v);
    b = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
    if (v != v) b = 0xffffffffu;
    return ((unsigned long long)b << 32) | (uint32_t)(0x7fffffff - i);
}

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t lo = __shfl_xor((uint32_t)v, o), hi = __shfl_xor((uint32_t)(v >> 32), o);
        const unsigned long long u = ((unsigned long long)hi << 32) | lo;
        v = u > v ? u : v;
    }
    return v;
}

__global__ __launch_bounds__(TOPK_THREADS) void softmax_topk_kernel(const float* __restrict__ logits, float* __restrict__ values,
                                                                   int* __restrict__ indices, int K, int k, int want_prob) {
    __shared__ unsigned long long s_key[2][TOPK_WAVES];
    __shared__ float s_sum[TOPK_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* row = logits + (long long)blockIdx.x * K;
    unsigned long long prev = ~0ull;
    float mx = 0.f, total = 1.f;
    for (int r = 0; r < k; ++r) {
        unsigned long long best = 0;
        for (int i = tid; i < K; i += TOPK_THREADS) {
            const unsigned long long key = topk_key(row[i], i);
            if (key < prev && key > best) best = key;
        }
        best = wave_max_u64(best);
        if (lane == 0) s_key[r & 1][wave] = best;
        __syncthreads();                             // the other parity is rewritten only behind the next round's barrier
        best = s_key[r & 1][0];
#pragma unroll
        for (int q = 1; q < TOPK_WAVES; ++q) best = s_key[r & 1][q] > best ? s_key[r & 1][q] : best;
        prev = best;
        int idx = 0x7fffffff - (int)(uint32_t)best;               // k <= K: every round finds an element ...
        idx = idx < K ? idx : K - 1;                              // ... and no address is ever formed from anything else
        const float v = row[idx];
        if (r == 0 && want_prob) {                   // the first selection is the row maximum: sum_j expf(l_j - max), fixed order
            mx = v;
            float s = 0.f;
            for (int i = tid; i < K; i += TOPK_THREADS) s += expf(row[i] - mx);
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
            if (lane == 0) s_sum[wave] = s;
            __syncthreads();
            total = s_sum[0];
#pragma unroll
            for (int q = 1; q < TOPK_WAVES; ++q) total += s_sum[q];
        }
        if (tid == 0) {
            values[(long long)blockIdx.x * k + r] = want_prob ? expf(v - mx) / total : v;
            indices[(long long)blockIdx.x * k + r] = idx;
        }
    }
}

// ---- top-k accuracy: is the label among the k best of its row?  No selection is kept, so k is unbounded. ------------------------
// rank = #{j : x[j] > x[label] or (x[j] == x[label] and j < label)}: the position of the label in the order of the kernel above
// for rows without NaN (ties by ascending index; -0 == +0).  One workgroup per row, one pass; counts[i] += 1 where rank < ks[i],
// counts[nk] += B (block 0).  A label outside [0, K) or a NaN at the label's logit: wrong for every k, still counted.
struct TopkKs {
    int k[MV_TOPK_MAX_KS];
};

__global__ __launch_bounds__(TOPK_THREADS) void topk_correct_kernel(const float* __restrict__ logits, const int* __restrict__ labels,
                                                                   unsigned long long* __restrict__ counts, int B, int K, TopkKs ks,
                                                                   int nk) {
    __shared__ int s_rank[TOPK_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (blockIdx.x == 0 && tid == 0) atomicAdd(&counts[nk], (unsigned long long)B);
    const int label = labels[blockIdx.x];
    if (label < 0 || label >= K) return;             // block-uniform
    const float* row = logits + (long long)blockIdx.x * K;
    const float xl = row[label];
    if (xl != xl) return;
    int rank = 0;
    for (int i = tid; i < K; i += TOPK_THREADS) {
        const float v = row[i];
        rank += (v > xl || (v == xl && i < label)) ? 1 : 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) rank += __shfl_xor(rank, o);
    if (lane == 0) s_rank[wave] = rank;
    __syncthreads();
    if (tid == 0) {
        rank = 0;
#pragma unroll
        for (int q = 0; q < TOPK_WAVES; ++q) rank += s_rank[q];
        for (int i = 0; i < nk; ++i)
            if (rank < ks.k[i]) atomicAdd(&counts[i], 1ull);
    }
}

}  // namespace mv

using namespace mv;

extern "C" {

int mv_softmax_topk_f32(const float* logits, float* values, int* indices, int B, int K, int k, int want_prob,
                        mv_stream_t stream) {
    MV_CHECK_ARG(logits && values && indices, "softmax_topk: NULL buffer");
    MV_CHECK_ARG(B > 0 && K >= 1 && K <= 65536, "softmax_topk: bad dimensions B=%d K=%d (1 <= K <= 65536)", B, K);
    MV_CHECK_ARG(k >= 1 && k <= K && k <= MV_TOPK_MAX_K, "softmax_topk: k=%d must be in 1 .. min(K=%d, %d)", k, K, MV_TOPK_MAX_K);
    MV_CHECK_ARG(want_prob == 0 || want_prob == 1, "softmax_topk: want_prob must be 0 or 1, got %d", want_prob);
    set_kernel_name("softmax_topk");
    hipLaunchKernelGGL(softmax_topk_kernel, dim3(B), dim3(TOPK_THREADS), 0, (hipStream_t)stream, logits, values, indices, K, k,
                       want_prob);
    MV_LAUNCH_CHECK();
    return MV_OK;
}

int mv_topk_correct_f32(const float* logits, const int* labels, unsigned long long* counts, int B, int K, const int* ks, int nk,
                        mv_stream_t stream) {
    MV_CHECK_ARG(logits && labels && counts && ks, "topk_correct: NULL buffer");
    MV_CHECK_ARG(B > 0 && K >= 1 && K <= 65536, "topk_correct: bad dimensions B=%d K=%d (1 <= K <= 65536)", B, K);
    MV_CHECK_ARG(nk >= 1 && nk <= MV_TOPK_MAX_KS, "topk_correct: nk=%d must be in 1 .. %d", nk, MV_TOPK_MAX_KS);
    TopkKs v = {};
    for (int i = 0; i < nk; ++i) {
        MV_CHECK_ARG(ks[i] >= 1, "topk_correct: k=%d must be at least 1", ks[i]);
        v.k[i] = ks[i];
    }
    set_kernel_name("topk_correct");
    hipLaunchKernelGGL(topk_correct_kernel, dim3(B), dim3(TOPK_THREADS), 0, (hipStream_t)stream, logits, labels, counts, B, K, v, nk);
    MV_LAUNCH_CHECK();
    return MV_OK;
}

}  // extern "C"
