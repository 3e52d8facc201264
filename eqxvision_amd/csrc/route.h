// Which matrix-core kernel serves a convolution or a Linear: the whole rule as pure host code.  No HIP header: this file compiles
// with a plain C++17 host compiler, so a stand-alone program can ask it about every shape of the model zoo without launching
// anything (tests/test_route_host.py replays tests/data/routes.json through it).  The launchers (igemm.hip, conv_fallback.hip) compute
// a Route here and execute it; the kernels' files keep only what needs HIP.
#pragma once
#include <stddef.h>
#include <stdio.h>
#include <string.h>

#include "../../include/eqxvision_amd.h"

namespace mv {

// The library passes get_flag, a stand-alone program its own map.  Dynamic keys ("ov:M:C:K:R:S:s") go through it too.
typedef int (*FlagFn)(const char* name);

struct ConvShape {
    int N, H, W, C, K, R, S, sh, sw, ph, pw, dh, dw, groups, act, in_dtype, out_dtype;
    bool has_residual;
    bool has_scale = true;           // names only: igemm8's 256 x 256 Linear without a scale vector is its own symbol ("lin")
    int Ho() const { return (H + 2 * ph - dh * (R - 1) - 1) / sh + 1; }
    int Wo() const { return (W + 2 * pw - dw * (S - 1) - 1) / sw + 1; }
    long long M() const { return (long long)N * Ho() * Wo(); }
    bool dense() const { return R == 1 && S == 1 && sh == 1 && sw == 1 && ph == 0 && pw == 0; }
};
// a Linear over M rows is a 1x1 convolution over an M x 1 image
inline ConvShape linear_shape(long long M, int N, int K, int act, int in_dtype, int out_dtype, bool has_residual, bool has_scale) {
    ConvShape s = {1, (int)M, 1, K, N, 1, 1, 1, 1, 0, 0, 1, 1, 1, act, in_dtype, out_dtype, has_residual};
    s.has_scale = has_scale;
    return s;
}

enum class Kern { generic, stream1x1, skinny, conv3x3c64_v2, igemm8, igemm2, igemm128, igemm128_oddc };
// tile: igemm8 1 = 256x256, 2 = 128 pixels x 256 channels, 3 = 256x128; igemm2 1 = 256x64, 2 = 256x128, 3 = 256x256; igemm128 /
// igemm128_oddc / stream1x1 the channel width BN of the tile; skinny 0 = bf16, 1 = the exact-fp32 kernel; generic 0 = scalar,
// 1 = conv_f32_mfma, 2 = conv_f32_lds_mfma.  0 for igemm8 / igemm2 in a sibling's route: the entry refuses the shape.
struct Route { Kern kern; int tile; };

// ---- the predicates, each next to the measurements behind its thresholds ------------------------------------------------------
inline bool mfma_dtypes(int in_dtype, int out_dtype) { return in_dtype == MV_BF16 && (out_dtype == MV_BF16 || out_dtype == MV_F32); }

inline int igemm_supported(int C, int K, int R, int S, int groups, int in_dtype, int out_dtype) {
    (void)R; (void)S;
    return mfma_dtypes(in_dtype, out_dtype) && groups == 1 && C % 64 == 0 && K % 8 == 0;
}

// Channel counts that are multiples of 8 but not of 64 (MobileNet-style widths: 16, 24, 32, 96, 144, 160 ...): the 128 x 128 /
// 128 x 64 kernel of igemm.hip with the last k-tile of every tap zero-filled past C.
inline int igemm_oddc_supported(int C, int K, int groups, int in_dtype, int out_dtype) {
    return mfma_dtypes(in_dtype, out_dtype) && groups == 1 && C % 8 == 0 && C % 64 != 0 && K % 8 == 0;
}

inline int stream1x1_supported(int C, int K, int in_dtype, int out_dtype, long long M, FlagFn flag) {
    // C = reduction length, K = output channels (igemm naming)
    // the narrow / odd widths (16 ... 248 in steps of 8: the expansions / projections of MobileNet / EfficientNet / RegNet stacks,
    // whose outputs dominate the bytes) came later: before, they ran on the 128 x 128 tile kernel with a zero-filled k-tile at
    // 1.2-1.8 TB/s.  Multiples of 8 that are not multiples of 16 take the KPAD variant (half-empty last k-step).
    const bool wide = C == 64 || C == 96 || C == 128 || C == 192 || C == 256;
    const int kc = (C + 15) / 16;
    const bool narrow = C % 8 == 0 && C >= 16 && C < 256 && !flag("no_stream_narrow") &&
                        (C % 16 == 0 || (kc >= 2 && kc <= 13) || kc == 15);
    return mfma_dtypes(in_dtype, out_dtype) && (wide || narrow) && K % 8 == 0 && M >= 8192;
}

inline int skinny_f32_supported(long long M, int C, int K, int in_dtype, int out_dtype, bool has_residual, FlagFn flag) {
    return in_dtype == MV_F32 && out_dtype == MV_F32 && !has_residual && M >= 1 && M <= 1024 && C % 8 == 0 && C >= 64 &&
           K >= 8 && !flag("force_generic");
}

inline int skinny_supported(long long M, int C, int K, int in_dtype, bool has_residual) {
    // C = reduction length, K = output channels (igemm naming)
    return in_dtype == MV_BF16 && !has_residual && M >= 1 && M <= 256 && C % 16 == 0 && C >= 64 && K >= 8;
}

inline int conv3x3c64_supported(int C, int K, int R, int S, int sh, int sw, int ph, int pw, int dh, int dw, int in_dtype,
                                int out_dtype, bool has_residual, long long M) {
    return C == 64 && K == 64 && R == 3 && S == 3 && sh == 1 && sw == 1 && ph == 1 && pw == 1 && dh == 1 && dw == 1 &&
           in_dtype == MV_BF16 && out_dtype == MV_BF16 && !has_residual && M >= 8192;
}

inline int igemm8_supported(long long M, int C, int K, int R, int S, long long x_bytes, long long w_bytes) {
    // 64-channel k-tiles; the tap mask is 32 bits; byte offsets are 31 bits (the out-of-range marker is bit 31)
    return C % 64 == 0 && C >= 64 && K % 8 == 0 && R * S <= 32 && M < (1LL << 31) - 256 && x_bytes < (1LL << 31) - (1 << 22) &&
           w_bytes < (1LL << 31);
}

// The rule of the ping-pong kernels (igemm8.hip).  Returns the tile: 0 = not this kernel family, 1 = 256 x 256,
// 2 = 128 pixels x 256 channels, 3 = 256 pixels x 128 channels.  Measured (tools/g8_bench.py, round 2, ViT / Swin / ResNet
// shapes at full and half batch): the 256 x 256 kernel wins from ~0.6 of a round of CUs up; below that the half-size tiles
// fill the chip; layers with <= 128 output channels take the 256 x 128 tile; reductions shorter than 4 k-tiles stay on the
// streaming / 128 x 128 kernels (prologue + epilogue of the big tiles dominate).
#ifndef MV_ROUTE_T256_MIN            // a test builds a mutant with another threshold: the recorded table must notice
#define MV_ROUTE_T256_MIN 150
#endif
inline int igemm8_wanted(long long M, int C, int K, int R, int S, FlagFn flag) {
    if (flag("no_igemm8")) return 0;
    const long long nk = (long long)R * S * (C / 64);
    if (nk < 4 || K < 96) return 0;
    const long long tm256 = (M + 255) / 256, tm128 = (M + 127) / 128;
    if (K <= 128) return tm256 >= 90 ? 3 : 0;
    const long long tn = (K + 255) / 256, t256 = tm256 * tn, t128 = tm128 * tn;
    // (a "rounds x relative tile time" refinement that prefers 128 x 256 tiles when the last round of big tiles is nearly empty
    //  -- ViT fc2 at half batch: 154 -> 144 us alone -- LOSES 5% on the whole model: with two graph lanes the other lane's
    //  kernels fill that round.  The plain threshold below is what tools/tune_tiles.py confirms on whole-model time.)
    if (t256 >= MV_ROUTE_T256_MIN) return 1;
    return t128 >= 40 ? 2 : 0;
}

// Two-way split-K of the half-size tiles (igemm8s_kernel): a launch that leaves half of the 256 CUs idle and has a reduction long
// enough for two main loops.  `tiles` = tiles of the 128 x 256 / 256 x 128 shape, `nk` = 64-channel k-tiles of the whole reduction.
inline bool splitk_rule(long long tiles, long long nk, FlagFn flag) {
    if (flag("no_splitk")) return false;
    // the hand-over costs ~8 us (two atomics, 128 KB out of one CU and into another): it pays from ~40 k-tiles up
    // (tools/time_splitk.py: 72 k-tiles x1.34, 48 x1.10-1.22, 32 x1.05, 12 x0.75)
    const int min_nk = flag("splitk_min_nk") ? flag("splitk_min_nk") : 40;
    const int max_tiles = 128;
    return tiles <= max_tiles && nk >= min_nk;
}
constexpr size_t SCRATCH_SYNC_BYTES = 4096;      // head of every scratch offer: split-K arrival words, zero between launches
constexpr size_t SPLITK_SYNC_BYTES = SCRATCH_SYNC_BYTES;            // 2 words x 512 tiles
constexpr const char* kSplitkSuffix = "_splitk"; // appended to an igemm8 launch's name once it has taken the caller's scratch
// the scratch an igemm8 launch of `tiles` half-size tiles takes if the caller offered it; 0 = this launch does not split
inline size_t splitk_need_bytes(long long tiles, long long nk, FlagFn flag) {
    return splitk_rule(tiles, nk, flag) ? SPLITK_SYNC_BYTES + (size_t)tiles * 128 * 256 * 4 : 0;
}

inline int igemm2_wanted(long long M, int C, int K, int R, int S) {
    // worth it once there is enough work to fill the chip with 256-row tiles and a reduction of >= 4 k-tiles
    const long long ktiles = (long long)R * S * (C / 64);
    (void)K;
    // (from M = 2048 when the reduction is long, >= 32 k-tiles: Swin stage-3 fc2 3072 -> 768 at M = 3136, +0.5% swin_t)
    return (M >= 4096 || (M >= 2048 && ktiles >= 32)) && ktiles >= 4 && R * S <= 64;
}

// block tile of igemm2 for (M rows, K output channels): 1 = 256x64, 2 = 256x128, 3 = 256x256; `forced` != 0 wins
inline int igemm2_tile_rule(long long M, int K, int forced) {
    if (forced) return forced;
    const long long big_tiles = ((M + 255) / 256) * (long long)((K + 255) / 256);
    return K <= 64 ? 1 : ((K >= 1024 && big_tiles >= 512) ? 3 : 2);
}

inline int igemm2_dual_supported(long long M, int C1, int C2, int K, int dtype, FlagFn flag) {
    return dtype == MV_BF16 && C1 % 64 == 0 && C2 % 64 == 0 && C1 >= 64 && C2 >= 64 && K % 8 == 0 && M >= 4096 &&
           M < (1LL << 31) - 256 && !flag("no_dual");
}

// the fp32 matrix-core variants of the generic convolution (conv_fallback.hip: conv_generic_dispatch); aligned4 = every stride of x
// and w is a multiple of 4 elements and the channel stride is 1
inline int generic_variant(bool all_f32, int groups, int C, int K, bool aligned4, long long M, FlagFn flag) {
    if (!all_f32 || groups != 1 || flag("no_f32_mfma") || flag("force_generic")) return 0;
    if (K >= 32 && C >= 64 && aligned4 && M >= 1024 && !flag("no_f32_lds")) return 2;
    return K >= 8 ? 1 : 0;
}

// Per-shape kernel choice: "ov:<M>:<C>:<K>:<R>:<S>:<stride>" flags (tools/tune_tiles.py sets them while it searches:
// greedy, one shape at a time, judged on whole-model ms/step in one process) and the short table of shapes where the
// search beat the rules below by more than its 0.4% threshold.  Choices: 1/2/3 = igemm2 256x64 / 256x128 / 256x256,
// 7 / 8 = 128x128 / 128x64 (igemm.hip), 9 = stream1x1, 10 / 11 / 12 = igemm8 256x256 / 128x256 / 256x128;
// 0 = the rules.  Kinds: "ov" conv / linear, "ovh" head-major qkv projection, "ovd" dual-source pointwise (3 = igemm2, 10 = igemm8).
// Round 1 (profiles/r01/*_tile_search.txt): resnet50 B=256 and swin_t B=128 -- nothing above the drift (+0.4% / -0.4%
// in total), rules kept; vit_base B=256, two lanes -- three shapes, +3.5% together:
struct TunedTile { const char* kind; int M, a, b, R, S, sh, choice; };
// Round 2: the three ViT-B rows of round 1 are gone -- igemm8 (choice 10, now the rule for those shapes) beats all of them.
// Round 3 (gpurun_out/r3d/tune_resnet50.log; after bneck_tail changed the mix): resnet50 B=256, two lanes -- two shapes, +2.2% and +1.6%
// (three more "wins" of that log are the rule's own kernel re-measured: drift)
// (inside the laned graph the other lane fills the idle CUs, so the per-FLOP cheaper 256-row tile wins although it leaves
// fewer tiles than CUs); swin_t B=128: nothing above the drift.
static const TunedTile kTuned[] = {
    {"ov", 25088, 1024, 256, 1, 1, 1, 10},    // layer-3 conv1 1x1 1024 -> 256 at 128 images: igemm8 256x256 (98 tiles) over 128x256 (196)
    {"ov", 6272, 512, 512, 3, 3, 1, 12},      // layer-4 conv2 3x3 at 128 images: igemm8 256x128
    {"ov", 21632, 192, 384, 3, 3, 1, 12},     // alexnet conv3 (13 x 13, 192 -> 384) at 128 images: igemm8 256x128 (+0.9%, gpurun_out/r3l/tune_alexnet.log)
};
inline int tile_override(const char* kind, long long M, int a, int b, int R, int S, int sh, FlagFn flag) {
    char key[96];
    snprintf(key, sizeof(key), "%s:%lld:%d:%d:%d:%d:%d", kind, M, a, b, R, S, sh);
    const int f = flag(key);
    if (f) return f > 0 ? f : 0;                          // a negative flag = "the rules", whatever the table says
    if (flag("no_tuned")) return 0;
    for (const TunedTile& t : kTuned)
        if (!strcmp(t.kind, kind) && t.M == M && t.a == a && t.b == b && t.R == R && t.S == S && t.sh == sh) return t.choice;
    return 0;
}

// ---- the rule ------------------------------------------------------------------------------------------------------------------
inline Route route128(Kern k, int K) { return {k, K <= 64 ? 64 : 128}; }
inline Route route_stream(int K) { return {Kern::stream1x1, K <= 64 ? 64 : 128}; }

// mv_conv2d_nhwc_fwd (and mv_linear_fwd through route_linear)
inline Route route_conv(const ConvShape& s, FlagFn flag) {
    const long long M = s.M();
    const int C = s.C, K = s.K, R = s.R, S = s.S;
    const bool dense = s.dense();
    const bool all_f32 = s.in_dtype == MV_F32 && s.out_dtype == MV_F32;       // (the weights have the input's type)
    const Route generic = {Kern::generic, generic_variant(all_f32, s.groups, C, K, C % 4 == 0, M, flag)};
    if (flag("force_generic")) return generic;
    // the streaming kernel: pointwise layers whose reduction it has a variant for (Swin C = 96 included); its epilogue has
    // every activation
    const bool stream_ok = dense && s.groups == 1 && stream1x1_supported(C, K, s.in_dtype, s.out_dtype, M, flag);
    const bool stream_on = stream_ok && !flag("no_stream") && !flag("igemm_tile");
    if (!igemm_supported(C, K, R, S, s.groups, s.in_dtype, s.out_dtype)) {
        if (stream_on) return route_stream(K);
        if (!flag("no_oddc") && igemm_oddc_supported(C, K, s.groups, s.in_dtype, s.out_dtype) && M < (1LL << 31) - 256)
            return route128(Kern::igemm128_oddc, K);                      // widths like 24 / 96 / 144 / 160: zero-filled last k-tile
        return generic;
    }
    if (s.act > MV_ACT_GELU_TANH) {
        // jax.nn.hard_swish / hard_sigmoid / sigmoid / silu (MobileNetV3, EfficientNet): besides the streaming kernel only igemm.hip's
        // epilogue implements them; fused there they save the element-wise pass over the layer's output that a faster main loop
        // would not buy back
        if (stream_on && !flag("igemm2_tile")) return route_stream(K);    // (igemm2_tile bars streaming here but not below: kept as found)
        return route128(Kern::igemm128, K);
    }
    const bool forced_old = flag("igemm_tile") || flag("igemm2_tile") || flag("no_igemm2");
    const int f8 = flag("igemm8");                                        // forced (tests): 2 = 256x256, 3 = 128x256, 4 = 256x128
    if (dense && !flag("no_skinny") && !forced_old && f8 < 2 && skinny_supported(M, C, K, s.in_dtype, s.has_residual))
        return {Kern::skinny, 0};                                         // classifier heads: one wave per 32 x 32 tile
    const bool ok8 = igemm8_supported(M, C, K, R, S, 2LL * s.N * s.H * s.W * C, 2LL * K * R * S * C);
    if (f8 >= 2 && f8 <= 4 && ok8) return {Kern::igemm8, f8 - 1};
    const bool plain = !forced_old && !flag("no_stream");
    const int ov = plain && s.sh == s.sw ? tile_override("ov", M, C, K, R, S, s.sh, flag) : 0;
    if (ov >= 1 && ov <= 3 && R * S <= 64) return {Kern::igemm2, ov};
    if (ov >= 10 && ov <= 12 && ok8) return {Kern::igemm8, ov - 9};       // (the table is read before no_igemm8: kept as found)
    if (ov == 9 && stream_ok) return route_stream(K);
    if (ov == 7) return {Kern::igemm128, 128};
    if (ov == 8) return {Kern::igemm128, 64};
    // (igemm_tile / igemm2_tile suppress conv3x3c64 but no_igemm2 does not: kept as found)
    if (!flag("no_stream") && !flag("igemm_tile") && !flag("igemm2_tile") &&
        conv3x3c64_supported(C, K, R, S, s.sh, s.sw, s.ph, s.pw, s.dh, s.dw, s.in_dtype, s.out_dtype, s.has_residual, M))
        return {Kern::conv3x3c64_v2, 0};
    if (stream_on) return route_stream(K);
    // The ping-pong kernels (igemm8.hip) are THE GEMM core: every layer its rule accepts (enough tiles of one of its three
    // shapes, a reduction of >= 4 k-tiles).  What is left below -- igemm2's 256-row tiles for short reductions, igemm.hip's
    // 128 x 128 tile for small / odd shapes -- is the long tail.
    const int t8 = forced_old ? 0 : igemm8_wanted(M, C, K, R, S, flag);
    if (t8 && ok8) return {Kern::igemm8, t8};
    // deep-pipelined 8-wave kernel (igemm2.hip): real convolutions (taps or stride) and big Linears the rule above passed on
    const long long dense_m = C >= 512 ? 4096 : 32768;
    const bool want2 = igemm2_wanted(M, C, K, R, S) && (!dense || M >= dense_m || s.out_dtype == MV_F32 || flag("igemm2_tile"));
    if (!flag("no_igemm2") && !flag("igemm_tile") && want2) return {Kern::igemm2, igemm2_tile_rule(M, K, flag("igemm2_tile"))};
    const int tile = flag("igemm_tile");
    return tile ? Route{Kern::igemm128, tile == 2 ? 64 : 128} : route128(Kern::igemm128, K);
}

// mv_linear_fwd
inline Route route_linear(const ConvShape& s, FlagFn flag) {
    if (skinny_f32_supported(s.M(), s.C, s.K, s.in_dtype, s.out_dtype, s.has_residual, flag))
        return {Kern::skinny, 1};                                         // fp32 classifier heads (exact-fp32 MFMA)
    return route_conv(s, flag);
}

// The head-major Linear, the dual-source pointwise and the split-precision Linear choose between igemm8 and igemm2 only.
// What differs between them: how the forced "igemm8" flag is treated, the override (read by the caller: its kind and key
// differ), and the shortest reduction the igemm8 RULE is asked about.  -> {igemm8, tile} or {igemm2, 0}.
enum class Forced8 { ignored, checked, unchecked };      // checked: a forced or chosen tile still needs igemm8_supported
inline Route route_gemm8_or_2(long long M, int C, int K, int ov, Forced8 forced, bool ok8, int min_ktiles, FlagFn flag) {
    int t8 = 0;
    if (forced != Forced8::ignored && flag("igemm8") >= 2) t8 = flag("igemm8") - 1;
    else if (ov >= 10 && ov <= 12) t8 = ov - 9;
    else if (ov == 0 && C / 64 >= min_ktiles) t8 = igemm8_wanted(M, C, K, 1, 1, flag);
    if (t8 && (ok8 || forced != Forced8::checked)) return {Kern::igemm8, t8};
    return {Kern::igemm2, 0};
}

// mv_linear_heads_fwd: y[M][N] = x[M][K] . w[N][K]^T, stored head-major
inline Route route_linear_heads(long long M, int N, int K, FlagFn flag) {
    const int ov = !flag("igemm2_tile") ? tile_override("ovh", M, N, K, 1, 1, 1, flag) : -1;
    Route r = route_gemm8_or_2(M, K, N, ov, Forced8::checked, igemm8_supported(M, K, N, 1, 1, 2LL * M * K, 2LL * N * K), 0, flag);
    if (r.kern == Kern::igemm2) r.tile = igemm2_tile_rule(M, N, ov == 2 || ov == 3 ? ov : flag("igemm2_tile"));
    return r;
}

inline int conv1x1_dual_supported(long long M, int C1, int C2, int K, int dtype, FlagFn flag) {
    return !flag("force_generic") && !flag("no_igemm2") && igemm2_dual_supported(M, C1, C2, K, dtype, flag);
}

// mv_conv1x1_dual_fwd: the reduction runs over two sources of C1 and C2 channels.  tile 0 = the entry refuses the shape.
inline Route route_conv1x1_dual(long long M, int C1, int C2, int K, int stride2, int dtype, FlagFn flag) {
    if (!conv1x1_dual_supported(M, C1, C2, K, dtype, flag)) return {Kern::igemm2, 0};
    const int ovd = tile_override("ovd", M, C1, C2, K, stride2, 1, flag);      // 10 / 11 / 12 = igemm8 tiles, 3 = igemm2, 0 = the rule
    // reductions shorter than 8 k-tiles: igemm2 (tuner, ResNet layer2 entry)
    Route r = route_gemm8_or_2(M, C1 + C2, K, ovd, Forced8::unchecked, false, 8, flag);
    // 256 x 256 tiles measured +2% on resnet50 B=256 over 256 x 128 (the reductions are short: 6-24 k-tiles, so fewer,
    // larger tiles amortise prologue and epilogue)
    if (r.kern == Kern::igemm2) r.tile = K % 256 == 0 ? 3 : 2;
    return r;
}

// mv_linear_split_fwd: [x | x] . [w_hi | w_lo]^T on the dual igemm8 kernels, whatever the rule says about the size
inline Route route_linear_split(long long M, int N, int K, FlagFn flag) {
    const Route r = route_gemm8_or_2(M, 2 * K, N, 0, Forced8::ignored, true, 0, flag);
    return r.kern == Kern::igemm8 ? r : Route{Kern::igemm8, N <= 128 ? 3 : 2};
}

// ---- the names (mv_last_kernel; tests and tools pin them) ----------------------------------------------------------------------
constexpr const char* kGrouped64Name = "igemm_grouped64_bf16_128x64";     // mv_conv2d_nhwc_grouped64_fwd: one kernel, no rule

inline const char* generic_kernel_name(int variant) {
    return variant == 2 ? "conv_f32_lds_mfma" : (variant == 1 ? "conv_f32_mfma" : "conv_generic");
}

// `dual`: the two-source forms of igemm8 / igemm2.  `splitk`: the igemm8 launch took the caller's scratch.  "" = refused.
inline const char* kernel_name(Route r, bool dense, const ConvShape& s, bool dual, bool splitk, FlagFn flag) {
    static thread_local char nm[64];
    const char* dc = dense ? "dense" : "conv";
    const bool f32out = s.out_dtype == MV_F32;
    switch (r.kern) {
    case Kern::generic:
        return generic_kernel_name(r.tile);
    case Kern::stream1x1:
        snprintf(nm, sizeof(nm), "stream1x1_bf16_bn%d_k%d", r.tile, s.C);
        return nm;
    case Kern::skinny:
        return r.tile ? "skinny_linear_f32_mfma" : "skinny_linear_mfma";
    case Kern::conv3x3c64_v2:
        return "conv3x3c64_halo";
    case Kern::igemm8: {
        if (r.tile == 0) return "";
        const char* t = r.tile == 2 ? "128x256" : (r.tile == 3 ? "256x128" : "256x256");
        // one name per kernel SYMBOL (template instance), so that a rocprofv3 summary row and a bench row are the same launches:
        // <tile>_{conv | dense | lin}[_f32out]  <->  igemm8_kernel<OutT, false, MODE> / igemm8s_kernel<OutT, ARR, false, DENSE>
        const bool fast = dense && !flag("no_i8_lin");
        const char* mode = !fast ? (dense ? "dense0" : "conv") : ((r.tile == 1 && !s.has_scale) ? "lin" : "dense");
        if (dual) snprintf(nm, sizeof(nm), "igemm8_dual_bf16_%s%s%s", t, f32out ? "_f32out" : "", splitk ? kSplitkSuffix : "");
        else snprintf(nm, sizeof(nm), "igemm8_bf16_%s_%s%s%s", t, mode, f32out ? "_f32out" : "", splitk ? kSplitkSuffix : "");
        return nm;
    }
    case Kern::igemm2:
        if (r.tile == 0) return "";
        if (dual) return r.tile == 3 ? "igemm2_dual_bf16_256x256" : "igemm2_dual_bf16_256x128";
        snprintf(nm, sizeof(nm), "igemm2_bf16_256x%d_%s", r.tile == 1 ? 64 : (r.tile == 3 ? 256 : 128), dc);
        return nm;
    case Kern::igemm128:
        snprintf(nm, sizeof(nm), "igemm_bf16_128x%d_%s%s", r.tile, dc, s.act > MV_ACT_GELU_TANH ? "_act" : "");
        return nm;
    case Kern::igemm128_oddc:
        snprintf(nm, sizeof(nm), "igemm_bf16_128x%d_%s_oddc", r.tile, dc);
        return nm;
    }
    return "";
}

}  // namespace mv
