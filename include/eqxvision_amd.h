/* eqxvision_amd -- C ABI of the MI355X (gfx950) forward-pass engine.
 *
 * The reference (paganpasta/eqxvision) has NO native/FFI interface: its hot path is
 * `jax.vmap(net, axis_name="batch")(images, key=keys)` (README.md:37-40) over
 * `eqx.Module.__call__`s that bottom out in equinox/jax ops.  This header is the boundary the
 * replacement sits behind; each entry point names the reference op(s) it replaces.  The Python
 * host (`eqxvision_amd/_lib.py`) binds it with ctypes; INTEGRATION.md shows the stub.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (hipMalloc / torch .data_ptr()), dense, caller-owned;
 *   - activations are NHWC ("pixel-major, channel-contiguous") or row-major [rows][features];
 *     the only NCHW tensors are user images entering `mv_conv2d_nchw_fwd` and the layout
 *     converters;
 *   - dtype codes: MV_F32 / MV_BF16.  bf16 = bf16 storage, fp32 accumulate, fp32 epilogue;
 *   - all work is enqueued on `stream` (a hipStream_t; NULL = default stream), asynchronous;
 *   - return 0 on success, negative MV_E_* on argument errors, positive = hipError_t;
 *     `mv_last_error()` gives a thread-local message.  Nothing aborts or throws across the ABI.
 */
#ifndef EQXVISION_AMD_H
#define EQXVISION_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MV_ABI_VERSION 2   /* 2 (round 6): mv_bottleneck_strip_* gone, mv_bn_train_dz_coef_f32 / mv_device_status / the layer-1 plan (rc0, rc, res, sub)
                            * chain entries and the LayerNorm-fold Linear pair (lnout / lnin) added, every scratch consumer keeps its data behind a 4096-byte sync header */

typedef void* mv_stream_t; /* hipStream_t */

enum { MV_F32 = 0, MV_BF16 = 1 };
/* Activations.  0-2 are fused into every GEMM / convolution epilogue.  3-6 (jax.nn.hard_swish / hard_sigmoid / sigmoid / silu:
 * mobilenetv3.py:57,72, efficientnet.py:117, lraspp.py:102) are implemented by mv_conv2d_nhwc_fwd (routed to the streaming kernel or
 * the one tile kernel whose epilogues have them), mv_conv2d_nchw_fwd (the image-entry kernels: the SiLU / hard-swish stems), the
 * depthwise convolution, mv_se_scale_fwd and the element-wise entries (mv_eltwise_fwd, mv_add_fwd, mv_channel_affine_fwd); every
 * other matrix-core entry refuses them with MV_E_INVALID. */
enum { MV_ACT_NONE = 0, MV_ACT_RELU = 1, MV_ACT_GELU_TANH = 2, MV_ACT_HARD_SWISH = 3, MV_ACT_HARD_SIGMOID = 4, MV_ACT_SIGMOID = 5,
       MV_ACT_SILU = 6 };
enum { MV_OK = 0, MV_E_INVALID = -1, MV_E_UNSUPPORTED = -2, MV_E_OOM = -3 };
/* mv_set_flag names (per calling thread; 0 = the tuned default).  Policy since round 4: ONE "no_<kernel>" switch per fused / special
 * kernel (in-process A/B with tools/ab_flag.py and the tests' cross-checks against the un-fused path), the forcing switches the tests
 * use to reach every tile shape, and nothing else -- switches whose A/B is settled are deleted together with the losing branch.
 *   cross-check     "force_generic" (every op on the simple VALU kernels)
 *   GEMM core       "igemm8" (2 / 3 / 4 = force 256x256 / 128x256 / 256x128 tiles), "no_igemm8", "no_i8_lin" (generic main loop for dense
 *                   1x1 / Linear shapes), "no_splitk", "splitk_min_nk" (tests: split short reductions too), "igemm2_tile" (1 / 2 / 3),
 *                   "no_igemm2", "igemm_tile" (1 / 2), "no_skinny", "no_tuned", "no_dual", and the per-shape choice
 *                   "ov:<M>:<C>:<K>:<R>:<S>:<stride>" / "ovh:<M>:<N>:<K>:1:1:1" / "ovd:<M>:<C1>:<C2>:<K>:<stride>:1" (tools/tune_tiles.py)
 *   streaming 1x1   "no_stream", "no_stream_narrow", "no_chain", "no_chain_stream", "no_dual_chain", "no_ln_stream", "ln_stream_192",
 *                   "no_chain_rc" (the layer-1 plan that leaves the first block output un-written: mv_conv1x1_chain_rc*_supported say no),
 *                   "no_chain_rc0" (host: first boundary on mv_conv1x1_dual_chain_fwd with y = NULL instead of mv_conv1x1_chain_rc0_fwd),
 *                   "no_chain_l2" (layer 2's streamed boundaries of chain_l2.hip off: today's dual GEMM / chain_stream / dense launches),
 *                   "no_chain_res" (last boundary on chain1x1's form), "no_chain_sub" (block output written whole, not sub-sampled),
 *                   "no_swin_precise" (host: plain bf16 block Linears for Swin widths off the fused kernels)
 *   whole blocks    "no_bneck_tail",
 *                   "no_ln_mlp", "ln_mlp_waves" (8 / 12 / 16), "no_ln_mlp_stream" (both also govern the _res entries),
 *                   "no_swin_block_attn", "swin_c96_shared" (the two-windows-per-workgroup kernel at C = 96), "no_patch_merge_ln",
 *                   "no_patch4_ln", "no_fc_stream", "no_cnblock_dw" (ConvNeXt blocks on the composition of the generic entries),
 *                   "no_swin_v2_fused" (host: Swin V2 blocks and patch merging on the literal composition -- LayerNorm, add and cast
 *                   launches instead of mv_layernorm_add_fwd; A/B with tools/time_swin_v2.py -- tools/ab_flag.py feeds 224 px images,
 *                   which 8 x 8 windows do not divide)
 *   entry / misc    "stem_v0", "no_stem_pool", "no_stem_pool11", "no_patch_f32out", "no_ln_slim", "no_grouped64", "no_dwconv",
 *                   "dwconv_generic", "dwconv_no_tile", "dwconv_tile3", "no_oddc", "no_se_fused", "se_fused_always", "eltwise_scalar",
 *                   "affine_scalar", "dropout_x8", "dropout_scalar", "no_f32_mfma" (fp32 contractions back on the VALU kernel), "no_f32_lds" (only the direct fp32 matrix-core kernel), "no_attn_f32_lds" (fp32 attention back on the one-wave-per-query kernels),
 *                   "wgrad_valu" / "dgrad_valu" (the one-thread-per-element gradient kernels: cross-check)
 * The debug build (EQV_PROF=1 python -m eqxvision_amd.build -> libeqxvision_amd_prof.so) additionally reads "prof_hi" / "prof_lo"
 * (a device buffer for per-wave phase stamps), "*_prof", "i8_skew", "i8_ablate", "strip_skew", "ln_mlp_dbg", "rc_dbg" (chain_rc ablations): none of them exists in
 * the product library. */

int mv_abi_version(void);
const char* mv_last_error(void);
int mv_set_flag(const char* name, int value);   /* flags are per calling THREAD, like mv_last_error */
int mv_get_flag(const char* name);
int mv_flags_epoch(void);                        /* hash of this thread's current switch settings (0 = all default): recorded launch lists key on it */
/* Device status word: kernels that detect a broken protocol at run time record it here instead of trapping (a trap poisons the whole
 * HIP context, graph replays and other streams included).  bit 0: a split-K block gave up waiting for its partner's partial sums
 * (dirty / shared scratch; the tile it wrote is incomplete).  bit 1: mv_softmax_xent_map_f32 met a label outside [0, C) on a counted
 * pixel (the pixel was left out; loss, gradient and sums of that call are not those of the labels given).  bit 2: mv_preprocess_u8_fwd / mv_preprocess_u8_ragged_fwd / mv_preprocess_u8_boxes_fwd was given a tap table (or a device record) that points outside the image or
 * outside what its geometry can need (the taps were clamped; the output of that call is not the resize asked for); mv_preprocess_u8_mix_fwd
 * sets it for a device record it had to clamp too.  bit 3: mv_preprocess_u8_mix_fwd met a device label outside [0, K) (it matched no class:
 * that row of the targets is not the one asked for).  Writes the word to *status, clears it if `clear`; SYNCHRONISES the
 * device -- call it where the host synchronises anyway (after a forward, at the end of a test). */
int mv_device_status(int clear, unsigned* status);
/* name of the kernel variant the last call on this thread dispatched to (for tests/bench) */
const char* mv_last_kernel(void);

/* eqx.nn.Conv2d (+ eqx.experimental.BatchNorm inference + relu + residual add), reference call
 * sites resnet.py:144-162, conv_norm_activation.py:60-85, alexnet.py:44-55.
 *   y[n,ho,wo,k] = act( scale[k] * sum_{r,s,c} x[n, ho*sh-ph+r*dh, wo*sw-pw+s*dw, c] * w[k,r,s,c]
 *                       + shift[k] + residual[n,ho,wo,k] )
 * x NHWC [N,H,W,C]; w KRSC [K][R][S][C/groups] (same dtype as x); scale/shift fp32 [K] or NULL
 * (=1 / =0); residual (out_dtype, NHWC like y) or NULL. */
int mv_conv2d_nhwc_fwd(const void* x, const void* w, const float* scale, const float* shift,
                       const void* residual, void* y,
                       int N, int H, int W, int C, int K, int R, int S,
                       int sh, int sw, int ph, int pw, int dh, int dw, int groups,
                       int act, int in_dtype, int out_dtype, mv_stream_t stream);

/* Same contraction for a raw NCHW image batch (the network entry: resnet.py:243-251 stem,
 * alexnet.py:44 conv1, patch_embed.py:60-62/79-82, swin.py:705-711).  x NCHW [N,C,H,W] of
 * x_dtype; w OIHW [K][C][R][S] of out_dtype; y NHWC rows of out_dtype.
 * Token mode (ViT): if tok_stride > 0 the output row of pixel p of image n is
 * n*tok_stride + tok_offset + p and `pos` (fp32 [tok_stride][K]) row tok_offset+p is added
 * (vit.py:269: concat(cls, x) + pos_embed).  Otherwise tok_stride = tok_offset = 0, pos NULL. */
int mv_conv2d_nchw_fwd(const void* x, const void* w, const float* scale, const float* shift, void* y,
                       int N, int C, int H, int W, int K, int R, int S,
                       int sh, int sw, int ph, int pw, int act, int x_dtype, int out_dtype,
                       int tok_stride, int tok_offset, const float* pos, mv_stream_t stream);

/* The same entry with bf16 operands and an fp32 result: the ViT patch embedding (patch_embed.py:60-62, vit.py:268-269) whose token
 * rows START the fp32 residual stream -- they are not rounded to bf16 on the way (and the cast pass disappears).  w OIHW bf16, y
 * fp32 rows; non-overlapping patches only (stride = kernel, no padding, S % 8 == 0): ask the _supported entry. */
int mv_conv2d_nchw_f32out_supported(int C, int H, int W, int K, int R, int S, int sh, int sw, int ph, int pw, int x_dtype);
int mv_conv2d_nchw_f32out_fwd(const void* x, const void* w, const float* scale, const float* shift, void* y, int N, int C,
                              int H, int W, int K, int R, int S, int sh, int sw, int ph, int pw, int act, int x_dtype,
                              int tok_stride, int tok_offset, const float* pos, mv_stream_t stream);

/* The ResNet network entry in one launch (resnet.py:243-254: conv1 -> bn1 -> relu -> maxpool):
 * x NCHW [N,C,H,W] of x_dtype, w OIHW, folded BN scale/shift, y NHWC [N][Po][Qo][K] with
 * (Ho, Wo) the convolution's and (Po, Qo) the MaxPool2d(pool_k, pool_s, pool_p) output size.  The conv map
 * never reaches HBM.  mv_stem_conv_pool_supported() says whether the configuration has the path
 * (C=3, K=64, 7x7/2 pad 3, pool 3/2 pad 1, ReLU, bf16 out); otherwise mv_conv2d_nchw_fwd +
 * mv_maxpool2d_nhwc_fwd. */
int mv_stem_conv_pool_supported(int C, int K, int R, int S, int sh, int sw, int ph, int pw,
                                int pool_k, int pool_s, int pool_p, int act, int x_dtype, int out_dtype,
                                int64_t in_elems);
int mv_stem_conv_pool_fwd(const void* x, const void* w, const float* scale, const float* shift, void* y,
                          int N, int C, int H, int W, int K, int R, int S, int sh, int sw, int ph, int pw,
                          int pool_k, int pool_s, int pool_p, int act, int x_dtype, int out_dtype,
                          mv_stream_t stream);

/* Two chained pointwise layers of consecutive ResNet bottlenecks in one launch (resnet.py:144-162: block i's
 * conv3 -> bn3 -> + identity -> relu, then block i+1's conv1 -> bn1 -> relu; blocks chained by nn.Sequential, :330-333):
 *   y [M,K]  = relu(scale3[k] * (x[M,C] . w3[K,C]^T) + shift3[k] + residual[M,K])
 *   t1[M,N2] = relu(scale1[n] * (y[M,K] . w1[N2,K]^T) + shift1[n])
 * All operands bf16, NHWC rows; y is rounded to bf16 before the second product, exactly as the un-fused pair
 * (two mv_conv2d_nhwc_fwd calls) would see it.  mv_conv1x1_chain_supported() says whether the shape has the path:
 * C=64, K=256, N2=64 or 128, M >= 8192 (both weight matrices resident in LDS), or C=128, K=512, N2=128, M >= 16384
 * (ResNet-50 layer2: the weights streamed through LDS in 32-channel chunks of y).  y must not alias x, residual or t1. */
int mv_conv1x1_chain_supported(int64_t M, int C, int K, int N2, int dtype);
int mv_conv1x1_chain_fwd(const void* x, const void* w3, const float* scale3, const float* shift3,
                         const void* residual, void* y, const void* w1, const float* scale1,
                         const float* shift1, void* t1, int64_t M, int C, int K, int N2, int dtype,
                         mv_stream_t stream);

/* The tail of an identity ResNet bottleneck, CU-resident per image (resnet.py:144-162: conv2 3x3 -> bn2 -> relu -> conv3 1x1 ->
 * bn3 -> + identity -> relu; stride 1, no downsample branch), one launch, one workgroup per image:
 *   t2[B,H,W,width] = relu(scale2 * conv3x3_pad1(t1[B,H,W,width], w2) + shift2)      (stays in LDS, rounded to bf16)
 *   y [B,H,W,cout]  = relu(scale3 * (t2 . w3[cout,width]^T) + shift3 + residual[B,H,W,cout])
 * Weights in FRAGMENT ORDER (prepared once by the caller, eqxvision_amd/ops.py:prep_bneck_tail): a wave owns 32 output
 * channels and fetches each k16-step of them as one 1 KB piece,
 *   w2f[wave 0..7][tap r*3+s][j 0..width/16-1][lane 0..63][e 0..7] = w2[k = 32*wave + lane%32][r][s][c = 16*j + 8*(lane/32) + e]
 *   w3f[chunk 0..cout/256-1][wave][j][lane][e]                     = w3[k = 256*chunk + 32*wave + lane%32][c = 16*j + 8*(lane/32) + e]
 * (w2 in KRSC, w3 [cout][width]).  Supported: bf16, 14x14 maps, width 256, cout 1024 (ResNet-50/101/152 layer3).  y must
 * not alias t1 or residual. */
int mv_bottleneck_tail_supported(int H, int W, int width, int cout, int dtype);
int mv_bottleneck_tail_fwd(const void* t1, const void* w2f, const float* scale2, const float* shift2, const void* w3f,
                           const float* scale3, const float* shift3, const void* residual, void* y, int B, int H, int W,
                           int width, int cout, int dtype, mv_stream_t stream);

/* conv3 + BN and the downsample conv + BN of a stage's first bottleneck (resnet.py:144-162, 295-303) as ONE GEMM over
 * the concatenated reduction: both add into the same output, so
 *   y[N,Ho,Wo,K] = act(scale[k] * (x[N,Ho,Wo,C1] . wcat[k, 0:C1] + x2[N, s*ho, s*wo, C2] . wcat[k, C1:C1+C2]) + shift[k])
 * with x2 the block input read at pixel stride s (1 or 2) and the two BatchNorm scales folded into wcat's rows by the
 * caller (scale = NULL, shift = shift3 + shift_d).  The identity map is neither written nor read.  C1, C2 % 64 == 0. */
int mv_conv1x1_dual_supported(int64_t M, int C1, int C2, int K, int dtype);
int mv_conv1x1_dual_fwd(const void* x, const void* x2, const void* wcat, const float* scale, const float* shift,
                        void* y, int N, int Ho, int Wo, int C1, int H2, int W2, int C2, int stride2, int K,
                        int act, int dtype, mv_stream_t stream);

/* The same chain for the FIRST bottleneck of a stage whose identity is a 1x1 stride-1 convolution of the block input
 * (downsample = conv + BN, resnet.py:295-303; ResNet-50 layer1): conv3 and the downsample conv accumulate into one
 * output, so they are one GEMM over the concatenated reduction,
 *   y [M,K]  = relu(scale[k] * ([x | x2][M,C1+C2] . wcat[K,C1+C2]^T) + shift[k]),   t1 as above,
 * with wcat = [scale3 * W3 | scale_d * W_d] (the two BatchNorm scales folded into the bf16 weight rows by the caller),
 * shift = shift3 + shift_d, scale = NULL.  The identity map is never materialised.  C1 = C2 = 64, K = 256, N2 = 64. */
int mv_conv1x1_dual_chain_supported(int64_t M, int C1, int C2, int K, int N2, int dtype);
int mv_conv1x1_dual_chain_fwd(const void* x, const void* x2, const void* wcat, const float* scale,
                              const float* shift, void* y, const void* w1, const float* scale1,
                              const float* shift1, void* t1, int64_t M, int C1, int C2, int K, int N2,
                              int dtype, mv_stream_t stream);

/* ---- a bottleneck stage whose block outputs are not all written (round 6; resnet.py:144-162, 295-303, 330-333).  Between the fused
 * boundaries above the 256-channel block output y_i is still written once and read once; in a stage of three bottlenecks
 * (ResNet-50 / 101 / 152 layer1) most of that traffic can go:
 *   (1) mv_conv1x1_dual_chain_fwd with y = NULL: block 0 stores only t1 of block 1 -- y0 is recomputed by (2);
 *   (2) mv_conv1x1_chain_rc_fwd: block 1's boundary WITHOUT y0 in memory.  It reads t2 (block 1's conv2 output), t2_prev (block 0's)
 *       and x0 (the stage input), recomputes  y0 = relu([t2_prev | x0] . wcat0^T + shift0)  exactly as (1) computed it (bf16-rounded),
 *       then  y = relu(t2 . (scale1 w3)^T + shift1 + y0)  and  t1 = relu(y . (scaleN w1n)^T + shiftN).  Every BatchNorm scale is folded
 *       into the bf16 weight rows by the caller (as wcat of (1) always was); the shifts enter through the matrix pipe.
 *       wfrag: the three (scaled) weight matrices in MFMA fragment order, 128 fragments of 1 KB -- per 32-channel chunk c of y: 8 of
 *       wcat0[32c.., :] (k16-steps of [t2_prev | x0]), 4 of scale1 w3[32c.., :], 4 of scaleN w1n[:, 32c..] as (k-step s, 32-row
 *       tile a2) with the reduction index in accumulator order (slot 8 fh + i <-> channel 32 c + 8 (2 s + i / 4) + 4 fh + i % 4); a
 *       fragment is [lane = 32 fh + r][8 bf16] = W[row0 + r][k0 + 8 fh ..].  shifts: 18 rows of 64 32-bit words -- rows 0-7 shift0
 *       of chunk c, 8-15 shift1 of chunk c, 16-17 shiftN of tile a2 -- word r < 32 = bf16 hi(v) | bf16 lo(v) << 16 of v = shift[row r]
 *       (hi + lo = v to 16 mantissa bits), words 32-63 zero.  C = 64, K = 256, N2 = 64, M >= 8192;
 *   (3) mv_conv1x1_chain_sub_fwd: the LAST block's boundary when the only other consumer of y is a stride-2 pointwise convolution
 *       (the next stage's downsample branch): as mv_conv1x1_chain_fwd with N2 = 128, but y_sub = [N][H/2][W/2][K] holds only the
 *       pixels with even (h, w) -- the strided consumer reads it with stride 1 (mv_conv1x1_dual_fwd, stride2 = 1).
 *   (1') mv_conv1x1_chain_rc0_fwd: (1) rebuilt in (2)'s style -- t1 = relu(relu([t2 | x0] . wcat0^T + shift0) . (scaleN w1n)^T + shiftN),
 *       wfrag = 96 fragments (per chunk: the 8 of wcat0, the 4 of scaleN w1n, as in (2)), shifts = 10 rows (0-7 shift0, 8-9 shiftN);
 *       nothing is staged for y, so eight waves per CU run instead of six (twelve fit, but leave no registers for the fragment ring
 *       and measured slower).  Same shapes as (2).
 *   (3') mv_conv1x1_chain_res_fwd: mv_conv1x1_chain_fwd / (3) in (2)'s style, for the boundary whose identity comes from memory:
 *       y = relu(t2 . (scale3 w3)^T + shift3 + residual)  (all pixels, or with sub = 2 only those with even (h, w), compactly),
 *       t1 = relu(y . (scaleN w1n)^T + shiftN).  wfrag = 8 x (4 + 2 N2 / 32) fragments (per chunk c: 4 of scale3 w3[32c.., :], then the
 *       scaled w1n fragments as (k-step s, 32-row tile a2) in accumulator order), shifts = 8 rows of shift3 + N2 / 32 rows of shiftN,
 *       both as in (2).  C = 64, K = 256, N2 = 128, N H W >= 8192.
 * The wfrag / shifts operands of (1'), (2), (3') and of mv_conv1x1_dual_chain_res_fwd are ONE layout: per 32-channel chunk c of y the
 * k16-step fragments of the rows 32c.. of every scaled matrix that accumulates into y, side by side along the reduction, then the next
 * conv1's; one block of K / 32 shift rows per accumulation (the sum where two matrices share one), then the next conv1's.  The Python
 * package packs all of them with ops.chain_acc_operands; the kernels read them through csrc/chain_acc.h. */
int mv_conv1x1_chain_res_supported(int N, int H, int W, int C, int K, int N2, int sub, int dtype);
int mv_conv1x1_chain_res_fwd(const void* t2, const void* residual, const void* wfrag, const void* shifts, void* y, void* t1, int N, int H,
                             int W, int C, int K, int N2, int sub, int dtype, mv_stream_t stream);
/* ---- a C = 128 / K = 512 stage (ResNet-50 / 101 / 152 layer2), weights streamed through LDS (csrc/chain_l2.hip): (3') also takes
 * C = 128, K = 512, N2 = 128 or 256 (the last boundary, into layer3's conv1), sub = 0 or 2, N H W >= 16384, wfrag = 16 x (8 + 2 N2 / 32)
 * fragments, shifts = 16 + N2 / 32 rows; and the stage's first boundary WITH its output stored:
 *   mv_conv1x1_dual_chain_res_fwd: y = relu([t2 | x] . wcat^T + shift) (wcat = [scale3 w3 | scale_d w_d], shift = shift3 + shift_d),
 *       t1 = relu(y . (scaleN w1n)^T + shiftN).  x is the map the downsample branch reads (the previous stage's output written
 *       sub-sampled), [M][C2].  wfrag = 16 x ((C1 + C2) / 16 + 2 N2 / 32) fragments, per chunk c of y the (C1 + C2) / 16 of wcat[32c.., :]
 *       then those of w1n as in (3'); shifts = 16 rows of shift + N2 / 32 rows of shiftN.  C1 = 128, C2 = 256, K = 512, N2 = 128,
 *       M >= 16384.  The flag "no_chain_l2" switches all of this stage's forms off (today's launches run). */
int mv_conv1x1_dual_chain_res_supported(int64_t M, int C1, int C2, int K, int N2, int dtype);
int mv_conv1x1_dual_chain_res_fwd(const void* t2, const void* x, const void* wfrag, const void* shifts, void* y, void* t1, int64_t M,
                                  int C1, int C2, int K, int N2, int dtype, mv_stream_t stream);
int mv_conv1x1_chain_rc_supported(int64_t M, int C, int K, int N2, int dtype);
int mv_conv1x1_chain_rc0_fwd(const void* t2, const void* x0, const void* wfrag, const void* shifts, void* t1, int64_t M, int C, int K,
                             int N2, int dtype, mv_stream_t stream);
int mv_conv1x1_chain_rc_fwd(const void* t2, const void* t2_prev, const void* x0, const void* wfrag, const void* shifts, void* y,
                            void* t1, int64_t M, int C, int K, int N2, int dtype, mv_stream_t stream);
int mv_conv1x1_chain_sub_supported(int N, int H, int W, int C, int K, int N2, int dtype);
int mv_conv1x1_chain_sub_fwd(const void* x, const void* w3, const float* scale3, const float* shift3, const void* residual,
                             void* y_sub, const void* w1, const float* scale1, const float* shift1, void* t1, int N, int H, int W,
                             int C, int K, int N2, int dtype, mv_stream_t stream);

/* eqx.nn.Linear under vmap / Linear2d (vit.py:64,74; mlps.py:60-64; resnet.py:356;
 * extensions_2d.py:31-50):  y[M,N] = act(scale[n]*(x[M,K] . w[N,K]^T) + shift[n] + residual[M,N]).
 * in_dtype = out_dtype = MV_F32 with M <= 1024 (the classifier heads: resnet.py:356, vit.py:273, swin.py:771) runs on the
 * exact-fp32 MFMA: the logits then carry no bf16 rounding of the pooled features or of the head weights. */
int mv_linear_fwd(const void* x, const void* w, const float* scale, const float* shift,
                  const void* residual, void* y, int64_t M, int N, int K,
                  int act, int in_dtype, int out_dtype, mv_stream_t stream);

/* The same Linear / entry convolution with SPLIT-PRECISION weights: the fp32 weight of the reference is carried as two bf16
 * terms, w ~ w_hi + w_lo (w_hi = bf16(w), w_lo = bf16(w - w_hi): ~16 mantissa bits), and the kernel accumulates both products
 * in fp32.  For the few layers whose weight rounding dominates the bf16 logit error -- layers that PRODUCE the residual stream
 * instead of adding a correction to it (Swin patch embedding swin.py:705-711 and patch merging swin.py:61-65): 1.4e-2 -> 8e-3
 * on swin_t.  mv_linear_split_fwd: w_hi_lo is [N][2K] = [w_hi row | w_lo row]; otherwise as mv_linear_fwd (bf16 x).
 * mv_conv2d_nchw_split_fwd: as mv_conv2d_nchw_fwd without token mode. */
int mv_linear_split_supported(int64_t M, int N, int K, int dtype);
int mv_linear_split_fwd(const void* x, const void* w_hi_lo, const float* scale, const float* shift, const void* residual,
                        void* y, int64_t M, int N, int K, int act, int in_dtype, int out_dtype, mv_stream_t stream);
int mv_conv2d_nchw_split_fwd(const void* x, const void* w_hi, const void* w_lo, const float* scale, const float* shift,
                             void* y, int N, int C, int H, int W, int K, int R, int S, int sh, int sw, int ph, int pw,
                             int act, int x_dtype, int out_dtype, mv_stream_t stream);

/* x * scale broadcast over the pixels of each image: the last line of SqueezeExcitation.__call__ (layers/squeeze.py:60),
 * `x * scale_activation(fc2(...))`.  x, y NHWC [N, HW, C]; s [N, C]; all of `dtype`. */
int mv_channel_scale_nhwc_fwd(const void* x, const void* s, void* y, int N, int64_t HW, int C, int dtype, mv_stream_t stream);

/* SqueezeExcitation's scale vector in one launch (layers/squeeze.py:47-60): scale[n, c] = act2(b2 + w2 . act1(b1 + w1 . mean_hw x[n]))
 * for an NHWC bf16 map x[N, HW, C]; w1 [S][C] and w2t [S][C] bf16 (the first 1x1 convolution's weights, the second's TRANSPOSED:
 * both read along C), b1 / b2 fp32 or NULL; scale
 * [N][C] bf16.  act1 / act2: any MV_ACT_* (relu / silu and sigmoid / hard_sigmoid in the reference's models).  Follow with
 * mv_channel_scale_nhwc_fwd.  Flag "no_se_fused": pool, two B-row GEMMs and activation passes as separate launches. */
int mv_se_scale_supported(int C, int S, int dtype);
int mv_se_scale_fwd(const void* x, const void* w1, const float* b1, const void* w2t, const float* b2, void* scale, int N, int64_t HW,
                    int C, int S, int act1, int act2, int dtype, mv_stream_t stream);

/* Depthwise Conv2d (groups == in_channels == out_channels: mobilenetv2.py:58-68 `ConvNormActivation(hidden, hidden,
 * groups=hidden)`) with the folded BatchNorm and the activation in the same pass.  w_rsc: the (C, 1, R, S) filters re-laid
 * by the caller to [R][S][C] (channel-contiguous taps); x, y NHWC bf16; scale / shift fp32 [C] or NULL. */
int mv_dwconv2d_supported(int C, int K, int groups, int R, int S, int in_dtype, int out_dtype);
int mv_dwconv2d_nhwc_fwd(const void* x, const void* w_rsc, const float* scale, const float* shift, void* y, int N, int H, int W,
                         int C, int R, int S, int sh, int sw, int ph, int pw, int dh, int dw, int act, int in_dtype, int out_dtype,
                         mv_stream_t stream);

/* Grouped Conv2d on the matrix cores (ResNeXt conv2: resnet.py:17-27 `groups`, :440-471 `groups=32, width_per_group=4 | 8`; RegNet:
 * regnet.py:49-70, group widths 8 ... 264), for C == K and Cg = C / groups with Cg % 8 == 0 or Cg | 64.  A tile of 64 output
 * channels n0 .. n0+63 reads the contiguous WINDOW of input channels of the groups it touches, starting at (n0 / Cg) * Cg.  The CALLER
 * expands the [K][R][S][Cg] filters to w64 [K][R][S][win], win = mv_conv2d_grouped64_window(C, groups) (the widest window, a
 * multiple of 64): w64[k][r][s][(k / Cg) * Cg - ((k / 64 * 64) / Cg) * Cg + i] = w[k][r][s][i], 0 elsewhere (for Cg | 64 this is the
 * block-diagonal 64 x 64 tile).  Everything else as mv_conv2d_nhwc_fwd. */
int mv_conv2d_grouped64_supported(int C, int K, int R, int S, int groups, int in_dtype, int out_dtype);
int mv_conv2d_grouped64_window(int C, int groups);
int mv_conv2d_nhwc_grouped64_fwd(const void* x, const void* w64, const float* scale, const float* shift, const void* residual,
                                 void* y, int N, int H, int W, int C, int K, int R, int S, int sh, int sw, int ph, int pw, int dh,
                                 int dw, int groups, int act, int in_dtype, int out_dtype, mv_stream_t stream);

/* LayerNorm folded into the Linear that consumes it (swin.py:572-578 `attn(norm1(x))` / `mlp(norm2(x))` feeding qkv / fc1;
 * extensions_2d.py:9-50), for short rows (K = 96: Swin stage 0, where the LayerNorm launch is a 115 MB round trip; K = 192 only
 * behind the "ln_stream_192" switch -- it loses there, see stream1x1.hip):
 *   y[m,:] = act( w . n(x[m,:]) + bias ),   n(x) = (x - mean) * rsqrt(var + eps)   (biased var)
 * with the LayerNorm affine folded by the caller (w = W . diag(gamma) bf16 [N][K], bias = b + W . beta fp32).
 * x is MV_F32 (the fp32 residual stream) or MV_BF16; y is MV_BF16. */
int mv_ln_linear_supported(int64_t M, int N, int K, int x_dtype, int out_dtype);
int mv_ln_linear_fwd(const void* x, const void* w, const float* bias, void* y, int64_t M, int N, int K, float eps, int act,
                     int x_dtype, int out_dtype, mv_stream_t stream);

/* The MLP half of a pre-norm block in ONE launch (swin.py:572-578 `x + stochastic_depth(mlp(norm2(x)))` in inference,
 * mlps.py:54-66, extensions_2d.py:9-28), for narrow rows whose two weight matrices fit in LDS (C = 96, hidden = 384: Swin
 * stage 0, where the hidden activations are 154 MB per 64 images):
 *   y[m,:] = x[m,:] + w2 . gelu_tanh( w1 . n(x[m,:]) + b1 ) + b2,   n(x) = (x - mean) * rsqrt(var + eps)   (biased var)
 * The LayerNorm affine is folded by the caller: w1 = W1 . diag(gamma) (bf16 [hidden][C]), b1 = b1 + W1 . beta (fp32);
 * w2 bf16 [C][hidden], b2 fp32.  x and y share x_dtype (MV_F32 = the fp32 residual stream, or MV_BF16); not in place. */
int mv_ln_mlp_supported(int64_t M, int C, int hidden, int x_dtype);
int mv_ln_mlp_fwd(const void* x, const void* w1, const float* b1, const void* w2, const float* b2, void* y, int64_t M, int C,
                  int hidden, float eps, int x_dtype, mv_stream_t stream);

/* The ATTENTION half of a Swin block in ONE launch, one workgroup per window (swin.py:572-578 first line, 90-255, 342-366:
 * x + proj(shifted_window_attention(qkv(LayerNorm(x)))); inference, no dropout):
 *   x, y: MV_F32 [B][Hf][Wf][C] (the fp32 residual stream), not in place.  Cyclic shift, window partition / reverse and the shift
 *   mask (-100) are index arithmetic; q / k / v and the attention output never leave LDS.
 * The caller folds the LayerNorm affine into the qkv weights (W . diag(gamma), b + W . beta) and hands the weights over in
 * FRAGMENT ORDER (a wave fetches each k16-step of a 32-channel tile as one 1 KB piece; prepared by eqxvision_amd/ops.py):
 *   wqkv_f[group g 0..2][tile t 0..3*HG-1][j 0..C/16-1][lane 0..63][e 0..7] = Wqkv'[row(g,t) + lane%32][16*j + 8*(lane/32) + e]
 *       with HG = heads/3 heads per group and row(g,t) = (t/HG)*C + 32*(HG*g + t%HG): q, k, v of heads HG*g .. HG*g+HG-1;
 *       bqkv[g][t][0..31] = the matching bias slice
 *   wp_f[tile t 0..C/32-1][j][lane][e] = Wproj[32*t + lane%32][16*j + 8*(lane/32) + e];   bp[C]
 *   bias64[heads][64][64] fp32: relative-position bias bias[h][query][key] padded to 64 x 64, -1e30 on key columns >= 49
 * Supported: heads of 32 channels, 7 x 7 windows, C = 384 / 192 / 96 (swin_t / swin_s stages 2 / 1 / 0: one / two / one window
 * per workgroup -- two at C = 96 under the flag swin_c96_shared; the windows of an image must divide by that). */
int mv_swin_block_attn_supported(int Hf, int Wf, int C, int heads, int wsh, int wsw, int x_dtype);
int mv_swin_block_attn_fwd(const void* x, const void* wqkv_f, const float* bqkv, const void* wp_f, const float* bp,
                           const float* bias64, void* y, int B, int Hf, int Wf, int C, int heads, int wsh, int wsw, int shh,
                           int shw, float eps, int x_dtype, mv_stream_t stream);

/* The same MLP half for rows too wide for the weights to live in LDS (Swin stages 1 / 2: C = 192 / 384, hidden = 4 C): both weight
 * matrices are STREAMED from L2 straight into registers, 128 / 64 token rows per workgroup, the hidden activations pass through LDS in chunks
 * of 256 units and never reach HBM.  Same formula and folding as mv_ln_mlp_fwd; the weights come in FRAGMENT ORDER (prepared once
 * by the caller, eqxvision_amd/ops.py:ln_mlp): a wave fetches each k16-step of its 32 output units as one 1 KB piece,
 *   w1f[chunk 0..hidden/256-1][wave 0..7][j 0..C/16-1][lane 0..63][e 0..7] = w1[u = 256*chunk + 32*wave + lane%32][c = 16*j + 8*(lane/32) + e]
 *   w2f[chunk][tile 0..C/32-1][j 0..15][lane][e]                        = w2[c = 32*tile + lane%32][u = 256*chunk + 16*j + 8*(lane/32) + e]
 * x, y: MV_F32 (the fp32 residual stream), not in place. */
int mv_ln_mlp_stream_supported(int64_t M, int C, int hidden, int x_dtype);
int mv_ln_mlp_stream_fwd(const void* x, const void* w1f, const float* b1, const void* w2f, const float* b2, void* y, int64_t M,
                         int C, int hidden, float eps, int x_dtype, mv_stream_t stream);

/* The same two MLP kernels with the residual taken from ANOTHER tensor (the ConvNeXt block, convnext.py:62-72:
 * res + layer_scale * (w2 . gelu(w1 . n(x) + b1) + b2), x = the 7x7 depthwise output of mv_cnblock_dw_fwd with normalize = 0):
 *   y[m,:] = res[m,:] + w2 . gelu_tanh( w1 . n(x[m,:]) + b1 ) + b2
 * The caller folds the LayerNorm affine into w1 / b1 as for mv_ln_mlp_fwd and layer_scale into fc2 (w2 = diag(ls) . W2 in fp32, then
 * one bf16 rounding; b2 = ls * b2).  res and y are MV_F32 [M][C] (the residual stream; y may not alias x).  mv_ln_mlp_res_*: C = 96,
 * x MV_F32 or MV_BF16, weights as mv_ln_mlp_fwd; mv_ln_mlp_stream_res_*: C = 192 / 384, x MV_F32, weights in the fragment order of
 * mv_ln_mlp_stream_fwd.  Supported exactly where the entries without _res are (the same switches). */
int mv_ln_mlp_res_supported(int64_t M, int C, int hidden, int x_dtype);
int mv_ln_mlp_res_fwd(const void* x, const void* res, const void* w1, const float* b1, const void* w2, const float* b2, void* y,
                      int64_t M, int C, int hidden, float eps, int x_dtype, mv_stream_t stream);
int mv_ln_mlp_stream_res_supported(int64_t M, int C, int hidden, int x_dtype);
int mv_ln_mlp_stream_res_fwd(const void* x, const void* res, const void* w1f, const float* b1, const void* w2f, const float* b2, void* y,
                             int64_t M, int C, int hidden, float eps, int x_dtype, mv_stream_t stream);

/* ConvNeXt block head (convnext.py:34-52: Conv2d(C, C, 7, padding=3, groups=C, bias) -> LayerNorm2d(C)) in one pass:
 *   d[b,h,w,c] = bias[c] + sum_{r,s<7} x[b, h+r-3, w+s-3, c] * w_rsc[r][s][c]      (zero padding, fp32 accumulation)
 *   normalize = 0: y = d (y_dtype MV_BF16 or MV_F32: the input of mv_ln_mlp_res_fwd / mv_ln_mlp_stream_res_fwd)
 *   normalize = 1: y = (d - mean_c d) * rsqrt(var_c d + eps), biased var, two passes over the kept d (y_dtype MV_BF16; the affine
 *                  is folded into the next Linear by the caller)
 * x NHWC [N][H][W][C], MV_F32 (the residual stream) or MV_BF16; w_rsc the (C, 1, 7, 7) filters re-laid to [7][7][C] bf16 (as for
 * mv_dwconv2d_nhwc_fwd); bias fp32 [C] or NULL; not in place.  Any C % 8 == 0 up to 1536, any H, W (maps smaller than the window
 * included).  Flag "no_cnblock_dw". */
int mv_cnblock_dw_supported(int C, int H, int W, int x_dtype, int y_dtype, int normalize);
int mv_cnblock_dw_fwd(const void* x, const void* w_rsc, const float* bias, void* y, int N, int H, int W, int C, float eps,
                      int normalize, int x_dtype, int y_dtype, mv_stream_t stream);

/* ShuffleNetV2 unit tail (shufflenetv2.py:44-112: depthwise 3x3 + BatchNorm -> 1x1 + BatchNorm + ReLU) in one launch, writing one
 * half of a unit output kept in the FOLDED layout [B][Ho][Wo][y_pitch] (eqxvision_amd/ops.py: shuffle_unit), and optionally the
 * pass-through half of a stride-1 unit:
 *   d[m, c]            = bf16( dw_scale[c] * sum_{r,s<3} x[b, stride*ho + r - 1, stride*wo + s - 1, c] * w_dw[r][s][c] + dw_shift[c] )
 *   y[m, y_off + n]    = relu( pw_scale[n] * sum_c W[n][c] d[m, c] + pw_shift[n] )   for n < N_real,  exact 0 for N_real <= n < N
 *   y[m, pass_off + i] = src[m, phys(i)]   for i < n_pass,  exact 0 for n_pass <= i < pass_pad   (src != NULL, stride 1; a bit copy)
 *   phys(i) = i / 2 for even i, P_src + i / 2 for odd i   (the previous unit's channel shuffle as an index into its folded output)
 * m = b*Ho*Wo + ho*Wo + wo, Ho = (H - 1) / stride + 1 (pad 1).  x NHWC [B][H][W][Cx] bf16, dense; w_dw [3][3][Cx] bf16 (as for
 * mv_dwconv2d_nhwc_fwd); dw_scale / dw_shift fp32 [Cx] or NULL; pw_scale / pw_shift fp32 [N] or NULL; src [B][Ho][Wo][src_pitch]
 * bf16.  Every other channel of y is left untouched.  The intermediate d stays in LDS; fp32 accumulation in both stages.
 * w_frag: the [N][Cx] 1x1 weight in the A-fragment order of v_mfma_f32_16x16x32_bf16, zero-padded to Np = N rounded up to 16 rows
 * and Kp = Cx rounded up to 32 columns (eqxvision_amd/ops.py: dwpw_fragments):
 *   w_frag[tile 0..Np/16-1][step 0..Kp/32-1][lane 0..63][e 0..7] = W[16*tile + lane%16][32*step + 8*(lane/16) + e]
 * Cx, N: multiples of 8 in 8 .. 512; y_pitch, y_off, pass_off, pass_pad, P_src, src_pitch: multiples of 8; stride 1 or 2; bf16 only.
 * Flag "no_shuffle_dwpw": _supported returns 0 (the caller composes mv_dwconv2d_nhwc_fwd + mv_conv2d_nhwc_fwd). */
int mv_shuffle_dwpw_supported(int Cx, int N, int stride, int H, int W, int in_dtype, int out_dtype);
int mv_shuffle_dwpw_fwd(const void* x, const void* w_dw, const float* dw_scale, const float* dw_shift, const void* w_frag,
                        const float* pw_scale, const float* pw_shift, void* y, int y_pitch, int y_off, int N, int N_real,
                        const void* src, int src_pitch, int P_src, int n_pass, int pass_off, int pass_pad, int B, int H, int W, int Cx,
                        int stride, int in_dtype, int out_dtype, mv_stream_t stream);

/* SqueezeNet Fire module, expand half (squeezenet.py:45-53): both expand convolutions, their ReLUs and the concatenation in one
 * launch; each half lands in its channel slice of the one output tensor:
 *   y[m, n]      = relu( b1[n] + sum_{c<S}        W1[n][c]       t[m, c] )                         for n < E1
 *   y[m, E1 + n] = relu( b3[n] + sum_{r,s<3, c<S} W3[n][c][r][s] t[b, h + r - 1, w + s - 1, c] )   for n < E3   (zero padding)
 * m = b*H*W + h*W + w.  t NHWC [B][H][W][S] bf16 (the squeeze output), y NHWC [B][H][W][E1 + E3] bf16, dense, not in place; b1 / b3
 * fp32 [E1] / [E3] or NULL; fp32 accumulation.  The tile of t and its one-pixel halo are staged in LDS once per workgroup (the padding
 * is zeros written to LDS) and every output-channel tile is computed from that copy.
 * w1_frag / w3_frag: the weights in the A-fragment order of v_mfma_f32_32x32x16_bf16 (eqxvision_amd/ops.py: fire_fragments), with
 * the reduction index k = (3 r + s) * S + c (k = c for the 1x1) and the rows of a 32-channel tile permuted so that a lane's 16
 * accumulator registers are 16 consecutive output channels:
 *   w_frag[tile 0..E/32-1][step 0..K/16-1][lane 0..63][e 0..7] = Wk[32*tile + chan(lane%32)][16*step + 8*(lane/32) + e]
 *   chan(p) = 16*((p/4)%2) + 4*(p/8) + p%4
 * S in {16, 32, 48, 64}; E1 == E3 in {64, 128, 192, 256}; any H, W >= 1 (up to 4096) whose tile and halo rows fit LDS
 * ((131 + 2 W) * (2 S + 16) <= 160 KiB); bf16 only.  Flags "no_fire_expand" / "force_generic": _supported returns 0 (the caller
 * composes mv_conv2d_nhwc_fwd twice + mv_copy_rows); "fire_expand_m256": the 256-pixel tile whatever the pixel count. */
int mv_fire_expand_supported(int S, int E1, int E3, int H, int W, int x_dtype, int y_dtype);
int mv_fire_expand_fwd(const void* t, const void* w1_frag, const float* b1, const void* w3_frag, const float* b3, void* y, int B,
                       int H, int W, int S, int E1, int E3, int x_dtype, int y_dtype, mv_stream_t stream);

/* GoogLeNet Inception module (googlenet.py:229-237), the pointwise convolutions: folded BatchNorm + ReLU, the output columns split
 * over one or two strided destinations so that a branch lands in its channel slice of the module's output:
 *   v[m, n] = relu( scale[n] * sum_{c<C} w[n][c] x[m][c] + shift[n] )        m < M, n < N
 *   n <  n0:  dst0[m * ld0 + c0 + n]        = v[m, n]
 *   n >= n0:  dst1[m * ld1 + c1 + (n - n0)] = v[m, n]
 * x bf16 [M][C] dense rows, w bf16 [N][C] (the stacked filters of the merged convolutions), scale / shift fp32 [N]; fp32 accumulation.
 * n0 == N with dst1 == NULL is the one-destination form.  C, N, n0, the offsets and the strides (in elements) are multiples of 16:
 * every row is written in 16-byte pieces; nothing outside the two slices is touched.  bf16 only, not in place.  Flags
 * "no_inception_fused" / "force_generic": _supported returns 0 (the caller composes mv_conv2d_nhwc_fwd + mv_copy_rows). */
int mv_conv1x1_split_supported(int C, int N, int n0, int ld0, int c0, int ld1, int c1, int x_dtype, int y_dtype);
int mv_conv1x1_split_fwd(const void* x, const void* w, const float* scale, const float* shift, void* dst0, int ld0, int c0, void* dst1,
                         int ld1, int c1, int64_t M, int C, int N, int n0, int x_dtype, int y_dtype, mv_stream_t stream);

/* GoogLeNet Inception module, the 3x3 convolutions of branches 2 and 3 (googlenet.py:206-220) in one launch: padding 1, stride 1, folded
 * BatchNorm + ReLU; convolution i reads channels [ct_i, ct_i + S_i) of t and writes channels [cy_i, cy_i + N_i) of y:
 *   y[m, cy_i + n] = relu( scale_i[n] * sum_{r,s<3, c<S_i} W_i[n][c][r][s] t[b, h + r - 1, w + s - 1, ct_i + c] + shift_i[n] )
 * m = b*H*W + h*W + w; t NHWC bf16 with rows of ldt elements, y NHWC bf16 with rows of ldy; the output slices do not overlap; not in
 * place; fp32 accumulation.  A workgroup stages 128 pixels of one slice with their halo in LDS (the padding is zeros written to LDS) and
 * computes one pair of 32-channel tiles of one convolution, so small maps still fill the machine with output-channel tiles.
 * w_i_frag: the A-fragment order of mv_fire_expand_fwd with the rows padded by zeros to a multiple of 32
 * (eqxvision_amd/ops.py: inception_fragments):
 *   w_frag[tile 0..ceil(N/32)-1][step 0..9 S/16-1][lane 0..63][e 0..7] = Wk[32*tile + chan(lane%32)][16*step + 8*(lane/32) + e]
 *   k = (3 r + s) * S + c,  chan(p) = 16*((p/4)%2) + 4*(p/8) + p%4
 * S_i, N_i, offsets and strides are multiples of 16; (131 + 2 W) * (2 max(S_0, S_1) + 16) <= 160 KiB; bf16 only.  Flags as above. */
int mv_conv3x3_pair_supported(int S0, int S1, int N0, int N1, int H, int W, int x_dtype, int y_dtype);
int mv_conv3x3_pair_fwd(const void* t, int ldt, int ct0, int S0, int ct1, int S1, const void* w0_frag, const float* scale0,
                        const float* shift0, const void* w1_frag, const float* scale1, const float* shift1, void* y, int ldy, int cy0,
                        int N0, int cy1, int N1, int B, int H, int W, int x_dtype, int y_dtype, mv_stream_t stream);

/* DenseNet (densenet.py:55-67, 106-133): the pre-activated pointwise convolution -- BatchNorm + ReLU IN FRONT of a 1x1 convolution, which
 * no producer can fold because every consumer of a feature has its own statistics -- with an optional 2 x 2 average in front of the
 * product and a strided source and destination:
 *   a[mo, c] = bf16( mean over the pool x pool window of  relu(s1[c] * x[pix * ldx + c] + h1[c]) )      c < C, pool in {1, 2}
 *   v[mo, n] = sum_c w[n][c] * a[mo, c]                                                                  fp32 accumulation
 *   y[mo * ldy + cy + n] = relu(s2[n] * v + h2[n]),  or v when s2 == h2 == NULL
 * x NHWC bf16 [B][H][W] with rows of ldx >= C elements; ONLY channels [0, C) of a row are read (the rest of a dense block's buffer
 * is not written yet).  pool = 2: the output map is floor(H/2) x floor(W/2) (AvgPool2d(2, 2); an odd last row / column is dropped), the
 * mean is taken in fp32 after affine + ReLU and before the rounding to bf16; averaging in front of the convolution instead of behind
 * it is exact algebra (both are linear) and divides the product by four.  H < pool or W < pool: MV_E_INVALID.  w bf16 [N][C], s1 / h1
 * fp32 [C], s2 / h2 fp32 [N] or both NULL.  C, N, ldx, ldy and cy are multiples of 16; bf16 only; not in place.  The dense-layer
 * bottleneck is pool = 1 with BatchNorm 2 folded into s2 / h2 and a dense y; a transition is pool = 2 with the identity, y = channels
 * [0, N) of the next block's buffer.  Flags "no_dense_fused" / "force_generic": _supported returns 0 (the caller composes
 * mv_channel_affine_fwd, mv_conv2d_nhwc_fwd, mv_copy_rows, mv_avgpool2d_nhwc_fwd). */
int mv_preact_conv1x1_supported(int C, int N, int ldx, int ldy, int cy, int pool, int x_dtype, int y_dtype);
int mv_preact_conv1x1_fwd(const void* x, int ldx, const float* s1, const float* h1, const void* w, const float* s2, const float* h2,
                          void* y, int ldy, int cy, int B, int H, int W, int C, int N, int pool, int x_dtype, int y_dtype,
                          mv_stream_t stream);

/* DenseNet dense layer, conv2 (densenet.py:44-52): a plain 3x3 convolution, padding 1, stride 1, into a channel slice -- no affine
 * step, no ReLU, negative values survive:
 *   y[m * ldy + cy + n] = sum_{r,s<3, c<S} W[n][c][r][s] t[b, h + r - 1, w + s - 1, c]       n < N, m = b*H*W + h*W + w
 * t NHWC bf16 with rows of ldt >= S elements, y NHWC bf16 with rows of ldy; not in place; fp32 accumulation.  w_frag: the A-fragment
 * order of mv_conv3x3_pair_fwd (eqxvision_amd/ops.py: inception_fragments; N = 48 pads to 64 rows and the upper half tile is never
 * stored).  S, N, the strides and cy are multiples of 16; (131 + 2 W) * (2 S + 16) <= 160 KiB; bf16 only.  A workgroup owns 128 pixels,
 * or 64 below 131072 pixels (flags "dense3x3_m64" / "dense3x3_m128": that tile whatever the count).  Flags "no_dense_fused" /
 * "force_generic": _supported returns 0. */
int mv_conv3x3_slice_supported(int S, int N, int H, int W, int x_dtype, int y_dtype);
int mv_conv3x3_slice_fwd(const void* t, int ldt, int S, const void* w_frag, void* y, int ldy, int cy, int N, int B, int H, int W,
                         int x_dtype, int y_dtype, mv_stream_t stream);

/* eqx.nn.AvgPool2d(kernel_size, stride) (densenet.py:128): floor-mode output size ((H - kh) / sh + 1), no padding, every window
 * full; NHWC, MV_F32 or MV_BF16, fp32 sums; not in place.  H < kh or W < kw: MV_E_INVALID. */
int mv_avgpool2d_nhwc_fwd(const void* x, void* y, int N, int H, int W, int C, int kh, int kw, int sh, int sw, int dtype,
                          mv_stream_t stream);

/* y[r, j] = x[r, idx[j]] over the channel axis of rows x C_in -> rows x C_out (the literal channel shuffle / split of ShuffleNetV2,
 * shufflenetv2.py:16-23, where the folded layout is not used).  idx: C_out device int32 (an index outside 0 .. C_in-1 gives 0);
 * MV_F32 or MV_BF16, any channel counts, not in place.  A bit copy. */
int mv_channel_gather_nhwc_fwd(const void* x, const int* idx, void* y, int64_t rows, int C_in, int C_out, int dtype, mv_stream_t stream);

/* eqx.nn.Linear over FEW rows with a big weight matrix -- the AlexNet / VGG classifiers (alexnet.py:62-70: Linear(9216, 4096),
 * Linear(4096, 4096), Linear(4096, classes), each behind `jax.vmap` = M rows) -- y[M][N] = act(x[M][K] . w^T + bias).  The layer is
 * bound by streaming w: w_frag is w in MFMA fragment order, prepared once by the caller (eqxvision_amd/ops.py:fc_fragments),
 *   w_frag[tile 0..ceil(N/32)-1][step 0..K/16-1][lane 0..63][e 0..7] = w[32*tile + lane%32][16*step + 8*(lane/32) + e]  (zero rows past N);
 * the reduction is split over the CUs and the fp32 partial sums are added in a fixed order (bit-reproducible) by a second launch.
 * x: MV_BF16 [M][K]; y: MV_BF16 or MV_F32 [M][N]; bias fp32 [N] or NULL; workspace: device memory of at least
 * mv_fc_stream_workspace(M, N, K) bytes, owned by the caller, free again when the call has completed on `stream`. */
int mv_fc_stream_supported(int64_t M, int N, int K, int in_dtype, int out_dtype);
int64_t mv_fc_stream_workspace(int64_t M, int N, int K);
int mv_fc_stream_fwd(const void* x, const void* w_frag, const float* bias, void* y, void* workspace, int64_t workspace_bytes, int64_t M,
                     int N, int K, int act, int in_dtype, int out_dtype, mv_stream_t stream);

/* Scratch memory for the NEXT launch this host thread issues on `stream`.  The library never allocates device memory; a Conv2d /
 * Linear whose output has too few tiles to fill the 256 CUs and whose reduction is long (ResNet layer 4: resnet.py:144-162 at
 * 7 x 7; Swin stage 3: swin.py:148-156, 280-300 at 49 tokens per image) is run as a two-way split over the reduction when the caller
 * provides room for the fp32 partial sums: the two halves of a tile run on two CUs, the half that finishes second adds the other's
 * partial tile to its own (a + b == b + a: the result does not depend on which one that is -- bit-reproducible) and runs the
 * usual epilogue.  mv_splitk_scratch_bytes(M, N, K_reduction) = the bytes such a launch wants for an [M] x [N] output reduced over
 * K_reduction = R * S * C (+ C2) elements, 0 when it would not split.  Protocol: the first 4096 bytes must be ZERO when the memory is
 * first handed over (the kernel leaves them zero again); the memory must stay valid until the launch has completed on `stream`, and
 * must not be shared with a launch that can run concurrently (another stream / another branch of a captured graph).  The hand-over
 * is consumed by the launch that uses it; one that does not split ignores it and LEAVES IT PENDING for the next entry on this
 * thread and stream, so a host that does not want that withdraws it (bytes = 0 / ptr = NULL).  Every consumer -- the backward
 * entries too (mv_colsum_f32, the weight gradient) -- keeps its data behind the first 4096 bytes and those stay zero, so a pending
 * offer is always a valid hand-over for whichever entry takes it.  Without scratch every launch runs un-split (same entry points,
 * same results to within fp32 summation order). */
int mv_set_scratch(void* ptr, int64_t bytes, mv_stream_t stream);
int64_t mv_splitk_scratch_bytes(int64_t M, int64_t N, int64_t K_reduction);

/* jax.image.resize(x, shape, method="bilinear") for up-sampling (segmentation/_utils.py:52-58: logits -> input resolution;
 * deeplabv3.py:66-72: the pooled ASPP branch back to the feature size): half-pixel centres, out-of-range taps dropped and the
 * rest renormalised (== clamped taps for the 2-tap kernel).  x NHWC [N,h,w,C]; y NHWC [N,H,W,C] or, with out_nchw, NCHW
 * [N,C,H,W] (the layout the reference returns).  H >= h and W >= w, else MV_E_UNSUPPORTED (the antialiased down-sampling
 * window is not on the path). */
int mv_resize_bilinear_nhwc_fwd(const void* x, void* y, int N, int h, int w, int C, int H, int W, int in_dtype, int out_dtype,
                                int out_nchw, mv_stream_t stream);

/* The label map of a dense head in one launch: labels[b][y][x] = the first index of the maximum over c of the value that
 * mv_resize_bilinear_nhwc_fwd (fp32 output) writes for (b, c, y, x) -- the same taps and the same interpolation expression, so
 * the result equals argmax over the class axis of that tensor, which is never written.  x NHWC [B,h,w,C], MV_F32 or MV_BF16;
 * labels uint8 [B,H,W].  Ties go to the lower class, a NaN beats every number and the first NaN wins (jnp.argmax).
 * MV_E_INVALID: a NULL buffer, a non-positive size, C > 256, an unknown dtype, H < h or W < w. */
int mv_resize_argmax_nhwc_fwd(const void* x, void* labels, int B, int h, int w, int C, int H, int W, int x_dtype,
                              mv_stream_t stream);

/* Classifier tail in one launch: the k largest of each row of logits fp32 [B][K], values fp32 [B][k] and indices int32 [B][k]
 * sorted by value descending, equal values by ascending index (jax.lax.top_k).  want_prob = 0: values are the selected logits,
 * bit for bit; want_prob = 1: values are softmax probabilities expf(v - max) / sum_j expf(l_j - max) in fp32.  -0 and +0 are
 * equal values; a NaN orders above every number (and makes the probabilities of its row NaN).  1 <= K <= 65536, 1 <= k <= min(K, 16), else MV_E_INVALID.  One workgroup per row, no scratch, no atomics:
 * repeated runs give the same bits. */
#define MV_TOPK_MAX_K 16
int mv_softmax_topk_f32(const float* logits, float* values, int* indices, int B, int K, int k, int want_prob,
                        mv_stream_t stream);

/* Scoring on the device (no counterpart in the reference; the rule of torchvision's reference segmentation ConfusionMatrix):
 * mat[t * C + p] += 1 for every pixel with target t and prediction p, mat uint64 [C][C] (rows = target).  A pixel counts iff
 * 0 <= t < C -- 255, any other value >= C and negative int32 targets do not.  Both entries ADD into mat; the caller zeroes it.
 * Integer atomics only: the result is exact and the same for every run.  One launch each.
 *   mv_confusion_from_logits: p = the label mv_resize_argmax_nhwc_fwd writes for the same logits (same code), which is not stored;
 *     logits NHWC [B,h,w,C] MV_F32 / MV_BF16, labels [B,H,W] uint8 (label_bytes 1) or int32 (4).
 *   mv_confusion_from_labels: p read from a second label map; pred and labels n elements each, uint8 or int32 independently, any
 *     byte alignment for uint8.  A pixel whose p is outside [0, C) has no cell and is not counted.
 * MV_E_INVALID: a NULL buffer, a non-positive size, C outside 1 .. 256, an unknown dtype or byte width, H < h or W < w, an
 * int32 map that is not 4-byte aligned. */
int mv_confusion_from_logits(const void* logits, const void* labels, unsigned long long* mat, int B, int h, int w, int C,
                             int H, int W, int logits_dtype, int label_bytes, mv_stream_t stream);
int mv_confusion_from_labels(const void* pred, const void* labels, unsigned long long* mat, long long n, int C,
                             int pred_bytes, int label_bytes, mv_stream_t stream);

/* Top-k accuracy counters in one launch: for every row of logits fp32 [B][K] with label l = labels[row] (int32),
 * rank = #{j : x[j] > x[l] or (x[j] == x[l] and j < l)} (the tie rule of mv_softmax_topk_f32); counts[i] += 1 where
 * rank < ks[i], i < nk, and counts[nk] += B.  counts: uint64 [nk + 1] on the device, ADDED to; ks: nk values on the HOST, read
 * during the call, each >= 1 and otherwise unbounded (nothing is selected, MV_TOPK_MAX_K does not apply).  A row whose label is
 * outside [0, K) or whose logit at the label is NaN is wrong for every k and still counted in counts[nk].
 * 1 <= K <= 65536, 1 <= nk <= MV_TOPK_MAX_KS, else MV_E_INVALID. */
#define MV_TOPK_MAX_KS 8
int mv_topk_correct_f32(const float* logits, const int* labels, unsigned long long* counts, int B, int K, const int* ks, int nk,
                        mv_stream_t stream);

/* rows x row_bytes strided copy (jnp.concatenate of NHWC maps along channels, deeplabv3.py:132-136: one call per source with
 * dst offset by the channels already placed).  Sizes and pitches in bytes, multiples of 2. */
int mv_copy_rows(const void* src, void* dst, int64_t rows, int64_t row_bytes, int64_t src_pitch, int64_t dst_pitch,
                 mv_stream_t stream);

/* Image preprocessing in one launch (torchvision's evaluation preset: Resize(antialias=True) -> CenterCrop -> ToTensor ->
 * Normalize): B uint8 images of one size, x [B,Hin,Win,3] or, with in_chw, [B,3,Hin,Win], are resized to Hr x Wr with the
 * separable triangle filter (half-pixel centres; support max(1, in / out) per axis, so it antialiases only when down-sampling and
 * is plain two-tap bilinear otherwise; weights normalised over the taps inside the image), the Hout x Wout box at (top, left) of
 * the resized image is kept, and y = acc * a[c] + b[c] (one fma; a = 1 / (255 std), b = -mean / std, fp32 [3]) is stored as
 * out_dtype (MV_F32 / MV_BF16), NCHW [B,3,Hout,Wout] or, with out_nhwc, [B,Hout,Wout,3].  Only the box is computed.
 * The filter is given as one DEVICE table per axis covering the outputs of the box only (tab_h: Hout entries, tab_w: Wout):
 *   int32 first[n] | int32 count[n] | fp32 weight[n][taps]    (taps_h / taps_w: the pitch, >= every count)
 * output i of the box is sum_k weight[i][k] * input[first[i] + k], k < count[i], all taps inside the input axis.  Sums are fp32
 * in tap order (columns first, then rows), no atomics: repeated runs give the same bits.  The kernel never forms an address
 * from a table entry that leaves the image or its LDS tile; a table that would have sets bit 2 (value 4) of mv_device_status.
 * MV_E_UNSUPPORTED: more than MV_PREPROCESS_MAX_TAPS taps on an axis (tables, or what Hin / Hr, Win / Wr need: down-sampling
 * beyond 11.5x), a box outside the resized image, a NULL buffer, x and y overlapping. */
#define MV_PREPROCESS_MAX_TAPS 24
int mv_preprocess_u8_fwd(const void* x, void* y, const void* tab_h, const void* tab_w, const float* a, const float* b, int B, int Hin,
                         int Win, int Hr, int Wr, int top, int left, int Hout, int Wout, int taps_h, int taps_w, int in_chw,
                         int out_dtype, int out_nhwc, mv_stream_t stream);

/* The same transform for B images of DIFFERENT sizes in one launch (decoded photographs: every file has its own size).  The
 * images lie tightly packed, at any byte alignment, in one uint8 buffer x of x_bytes bytes; the tables of all images and axes lie
 * in one int32 buffer tab of tab_words words, each in the layout above; one record per image says where:
 *   offset        byte offset of the image in x ([Hin,Win,3] or, with in_chw, [3,Hin,Win])
 *   Hin, Win      its size;  Hr, Wr: the size it is resized to;  top, left: where the Hout x Wout box starts in the resized image
 *   tab_h, tab_w  word offsets in tab of its row table (Hout entries, pitch mh) and its column table (Wout entries, pitch mw)
 * Hout x Wout, in_chw, out_dtype, out_nhwc, a and b are per launch; y is [B,3,Hout,Wout] or [B,Hout,Wout,3].  The arithmetic of
 * an output is that of mv_preprocess_u8_fwd, so an image gives the bits it gives alone, whatever shares the launch with it.
 * The records are passed twice with the same contents.  rec_host (HOST memory, read before the call returns) is validated in
 * full -- image inside x, tables inside tab, box inside the resized image, taps, x and y not overlapping: MV_E_INVALID or
 * MV_E_UNSUPPORTED with a message that names the image, nothing launched -- and sizes the launch.  rec_dev (DEVICE memory) is
 * what the kernel reads, and it trusts it no more than the tables: a device record that leaves either buffer or exceeds the
 * pitches of the host copy stores nothing for its image, a table entry that leaves the image is clamped; both set bit 2 of
 * mv_device_status.
 * LDS rule: the grid is (tiles_x, tiles_y, B) with ONE tile and ONE LDS size, the largest tile of mv_preprocess_u8_fwd's list
 * whose staged rectangle fits 64 KiB for the largest row span, column span and table pitches any image of the batch needs.  One
 * steeply down-sampled image therefore gives the whole launch its small tile and its occupancy. */
typedef struct mv_preprocess_image {
    int64_t offset;
    int32_t Hin, Win, Hr, Wr, top, left, tab_h, tab_w, mh, mw;
} mv_preprocess_image;                           /* 48 bytes, no padding */
int mv_preprocess_u8_ragged_fwd(const void* x, int64_t x_bytes, void* y, const mv_preprocess_image* rec_host,
                                const mv_preprocess_image* rec_dev, const void* tab, int64_t tab_words, const float* a,
                                const float* b, int B, int Hout, int Wout, int in_chw, int out_dtype, int out_nhwc,
                                mv_stream_t stream);

/* The training transform in one launch (torchvision's RandomResizedCrop -> RandomHorizontalFlip -> ToTensor -> Normalize, the
 * random draws made by the caller): image i of a packed buffer x (as above: any sizes, one record each) is CROPPED to the h x w
 * box at (top, left) of its SOURCE pixels, the box is resized to Hout x Wout, mirrored left-right if flip != 0, and stored as
 * y = acc * a[c] + b[c] like mv_preprocess_u8_fwd (same layouts, dtypes and epilogue).  The filter is that entry's -- half-pixel
 * centres, support max(1, n_box / n_out), triangle weights normalised over the taps present -- with "present" meaning inside the
 * BOX: the result has the bits of a call on the box copied out as an image of its own.  There are no tables: the kernel
 * generates each tile's filter in float64 (centre s = (o + 0.5) n_box / n_out - 0.5; first = floor(s - sup) + 1 and
 * last = ceil(s + sup) - 1 clipped to the box; weights 1 - |x - s| / sup in ascending tap order, summed in that order, each
 * quotient rounded once to fp32), so a weight is within one fp32 rounding of the float64 value.  Output column j of a mirrored
 * image is the unmirrored column Wout - 1 - j, taps and tap order unchanged.  No atomics, sums in tap order: same bits every run.
 * rec_host (HOST memory) is validated in full before anything is launched -- image inside x, box non-empty and inside its image
 * (MV_E_INVALID), at most MV_PREPROCESS_MAX_TAPS taps per axis, min(n_box, int(2 max(1, n_box / n_out) + 1)), and x and y not
 * overlapping (MV_E_UNSUPPORTED), each message naming the image -- and sizes the one tile of the launch by the LDS rule of the
 * ragged entry.  rec_dev (DEVICE memory, same contents) is what the kernel reads; it forms no address from it unchecked: a record
 * whose image leaves x stores nothing, a box that leaves its image is clamped into it, tap counts are clamped to the pitches of
 * the launch; each sets bit 2 of mv_device_status. */
typedef struct mv_preprocess_box {
    int64_t offset;                                  /* byte offset of the image in x */
    int32_t Hin, Win, top, left, h, w, flip, pad;    /* box in SOURCE pixels; flip != 0: mirror left-right */
} mv_preprocess_box;                                 /* 40 bytes, no padding */
int mv_preprocess_u8_boxes_fwd(const void* x, int64_t x_bytes, void* y, const mv_preprocess_box* rec_host,
                               const mv_preprocess_box* rec_dev, const float* a, const float* b, int B, int Hout, int Wout,
                               int in_chw, int out_dtype, int out_nhwc, mv_stream_t stream);

/* The rest of the classification recipe in the training launch (torchvision's reference RandomMixup / RandomCutmix on the batch,
 * RandomErasing(value=0) per image, label smoothing; the random draws made by the caller).  x, rec_host / rec_dev, a, b, the
 * layouts and the dtypes are those of mv_preprocess_u8_boxes_fwd; image i has a second record, mv_preprocess_mix.  Rectangles are in
 * OUTPUT pixels, half-open, (y0, x0, y1, x1); y1 <= y0 or x1 <= x0 is empty and means none.
 *   v_i(p): the fp32 value mv_preprocess_u8_boxes_fwd gives image i at output pixel p with box record i before the output is
 *           rounded -- same generated filter, tap order, two passes and fma(acc, a[c], b[c]) -- or exactly 0.0f where p lies inside
 *           image i's OWN erase rectangle (erasing follows Normalize and precedes the mix, so it shows wherever image i is read,
 *           as itself or as somebody's partner).
 *   With r = partner[i]:  p inside image i's cut rectangle and r != i: y = v_r(p);  otherwise r == i or lam == 1: y = v_i(p);
 *           otherwise y = fadd(fmul(lam, v_i(p)), fmul(oml, v_r(p))): two rounded products, one rounded sum, no contraction.
 *   A bf16 output is rounded once, at the store.
 * A tile resamples only what it needs, decided per tile from the records: not the partner where lam == 1 and the tile lies outside
 * the cut rectangle; not itself where the tile lies inside it; neither image where that image's erase rectangle holds the tile.
 * Targets, by extra workgroups of the same launch: with s(y, k) = (k == y ? on : off),
 *   targets[i][k] = fadd(fmul(lam_t, s(labels[i], k)), fmul(oml_t, s(labels[r], k))), fp32 [B, K]; the caller passes
 *   on = fl32(1 - eps + eps / K), off = fl32(eps / K) for label smoothing eps.  labels_dev: int32 [B] in DEVICE memory;
 *   labels_host: the same in HOST memory or NULL (labels that exist on the device only).  labels_dev == NULL and targets == NULL
 *   together: no targets.  No atomics on data, nothing shared between workgroups: same bits every run.
 * rec_host, mix_host and labels_host (HOST memory) are validated in full before anything is launched, each message naming the
 * image.  MV_E_INVALID: what mv_preprocess_u8_boxes_fwd refuses in a box record; partner outside [0, B); a rectangle coordinate
 * outside [0, Hout] / [0, Wout]; lam, oml, lam_t or oml_t not finite or outside [0, 1]; a host label outside [0, K); labels without
 * targets or the reverse.  MV_E_UNSUPPORTED: more than MV_PREPROCESS_MAX_TAPS taps on an axis; x, y and targets overlapping.
 * The one tile of the launch follows the LDS rule of the ragged entry, with TH x 3 x TW fp32 more when any image has a partner: a
 * tile that needs both images runs the passes for the partner, keeps its results there, then runs them for itself.
 * rec_dev / mix_dev / labels_dev (DEVICE memory) are what the kernel reads; it forms no address from them unchecked: box records as
 * in the boxes entry; a partner outside [0, B), one whose image leaves x, or one in a launch whose host records had no partner is
 * treated as none; rectangles are clamped to the output; each sets bit 2 of mv_device_status.  A device label outside [0, K)
 * matches no class (off everywhere) and sets bit 3. */
typedef struct mv_preprocess_mix {
    int32_t partner;                 /* index of the image mixed in; == own index: none */
    float lam, oml;                  /* weights of this image and of the partner in the pixel mix */
    int32_t cy0, cx0, cy1, cx1;      /* cut rectangle: the partner's pixels replace this image's */
    int32_t ey0, ex0, ey1, ex1;      /* erase rectangle of THIS image */
    float lam_t, oml_t;              /* weights of the two labels in the targets */
} mv_preprocess_mix;                 /* 52 bytes, no padding */
int mv_preprocess_u8_mix_fwd(const void* x, int64_t x_bytes, void* y, const mv_preprocess_box* rec_host,
                             const mv_preprocess_box* rec_dev, const mv_preprocess_mix* mix_host, const mv_preprocess_mix* mix_dev,
                             const float* a, const float* b, const int32_t* labels_host, const int32_t* labels_dev, float* targets,
                             int K, float on, float off, int B, int Hout, int Wout, int in_chw, int out_dtype, int out_nhwc,
                             mv_stream_t stream);

/* The segmentation training transform in one launch (torchvision's segmentation preset: RandomResize -> RandomHorizontalFlip ->
 * RandomCrop with pad-if-smaller -> ToTensor -> Normalize, the random draws made by the caller): image i of a packed buffer x and
 * its label map in a packed buffer m (one record each) are resized WHOLE to Hr x Wr, mirrored left-right if flip != 0, padded on
 * the right and bottom to max(Hr, Hout) x max(Wr, Wout), and the Hout x Wout window at (top, left) of that padded image is stored.
 * Output pixel (i, j): r = top + i, q = left + j.  r >= Hr or q >= Wr: y = fma((float)image_fill, a[c], b[c]), labels = mask_fill.
 * Otherwise, with the resized column c' = flip ? Wr - 1 - q : q, y is the value of mv_preprocess_u8_boxes_fwd's generated filter
 * for resizing Hin x Win to Hr x Wr at (r, c') -- same taps, same tap order, same two passes and epilogue, so it has the bits of
 * that entry on the whole image -- and labels = m[(2 r + 1) Hin / (2 Hr)][(2 c' + 1) Win / (2 Wr)], integer division in 64 bits:
 * the centre-based nearest rule (PIL, torch's "nearest-exact"), on the half-pixel grid of the image filter.
 * y is [B,3,Hout,Wout] or [B,Hout,Wout,3], MV_F32 or MV_BF16; labels int32 [B,Hout,Wout], what mv_softmax_xent_map_f32 reads.
 * m == NULL and labels == NULL together: the image only.  No atomics, nothing shared between workgroups: same bits every run.
 * rec_host (HOST memory) is validated in full before anything is launched, each message naming the image.  MV_E_INVALID: image or
 * mask outside its buffer; Hin, Win, Hr or Wr < 1; top < 0, left < 0, top + Hout > max(Hr, Hout) or left + Wout > max(Wr, Wout);
 * m without labels or the reverse; a fill outside [0, 255].  MV_E_UNSUPPORTED: more than MV_PREPROCESS_MAX_TAPS taps on an axis,
 * min(n_in, int(2 max(1, n_in / n_out) + 1)); an output overlapping an input or the other output.  The one tile of the launch
 * follows the LDS rule of the ragged entry.  rec_dev (DEVICE memory, same contents) is what the kernel reads; it forms no address
 * from it unchecked: a record whose image or mask leaves its buffer stores nothing for that image, sizes and origins are clamped
 * into range, tap counts are clamped to the pitches of the launch; each sets bit 2 of mv_device_status. */
typedef struct mv_preprocess_seg {
    int64_t offset;        /* byte offset of the image in x ([Hin,Win,3] or, with in_chw, [3,Hin,Win]) */
    int64_t mask_offset;   /* byte offset of the mask in m ([Hin,Win] uint8); ignored when m is NULL */
    int32_t Hin, Win;      /* source size */
    int32_t Hr, Wr;        /* size the WHOLE image is resized to */
    int32_t top, left;     /* origin of the Hout x Wout window in the padded image */
    int32_t flip, pad;     /* flip != 0: mirror left-right after the resize, before padding */
} mv_preprocess_seg;       /* 48 bytes, no padding */
int mv_preprocess_u8_seg_fwd(const void* x, int64_t x_bytes, const void* m, int64_t m_bytes, void* y, int32_t* labels,
                             const mv_preprocess_seg* rec_host, const mv_preprocess_seg* rec_dev, const float* a, const float* b,
                             int B, int Hout, int Wout, int image_fill, int mask_fill, int in_chw, int out_dtype, int out_nhwc,
                             mv_stream_t stream);

/* eqx.nn.MaxPool2d (resnet.py:254, alexnet.py:46,49,56): -inf padding, floor output size. */
int mv_maxpool2d_nhwc_fwd(const void* x, void* y, int N, int H, int W, int C,
                          int kh, int kw, int sh, int sw, int ph, int pw, int dtype, mv_stream_t stream);

/* eqx.nn.MaxPool2d(use_ceil=True) (squeezenet.py:88-112): the same pooling with the output size Ho x Wo given by the caller.  Per
 * axis it must be the floor size or the ceil size (floor + 1 where (size + 2 pad - kernel) % stride != 0: equinox grows the right /
 * bottom padding by `stride`), and the last window must still hold a tap of the map: MV_E_INVALID otherwise.  Taps outside the map
 * are skipped.  MV_F32 or MV_BF16. */
int mv_maxpool2d_out_nhwc_fwd(const void* x, void* y, int N, int H, int W, int C, int kh, int kw, int sh, int sw, int ph, int pw,
                              int Ho, int Wo, int dtype, mv_stream_t stream);

/* eqx.nn.AdaptiveAvgPool2d (resnet.py:283, alexnet.py:59, swin.py:757), equinox chunking rule. */
int mv_adaptive_avgpool2d_nhwc_fwd(const void* x, void* y, int N, int H, int W, int C, int oh, int ow,
                                   int in_dtype, int out_dtype, mv_stream_t stream);

/* eqx.nn.LayerNorm under vmap / LayerNorm2d (vit.py:149,154,272; extensions_2d.py:9-28):
 * M rows of C, biased variance, gamma/beta fp32 [C] or NULL.  Row i of x starts at element
 * i*x_row_stride (0 = dense = C), so e.g. only the cls row of every image can be normalised
 * (vit.py:272-273 uses x[0] only); y is dense [M][C]. */
int mv_layernorm_fwd(const void* x, const float* gamma, const float* beta, void* y,
                     int64_t M, int C, int64_t x_row_stride, float eps, int in_dtype, int out_dtype,
                     mv_stream_t stream);

/* _VitAttention core (vit.py:65-73): qkv [B,N,3,H,dh] (the qkv Linear output, channel order
 * [q|k|v][head][dh]) -> out [B,N,H*dh] = merge_heads(softmax(q k^T * scale) v);
 * probs (fp32 [B,H,N,N]) optional (NULL) -- the `attn` the reference returns. */
int mv_mha_fwd(const void* qkv, void* out, float* probs, int B, int N, int H, int dh, float scale,
               int dtype, mv_stream_t stream);

/* The same two reference lines (vit.py:64 qkv = self.qkv(x); vit.py:65-66 reshape + transpose to
 * [3, H, N, dh]) with the transposed layout produced by the projection itself: the GEMM epilogue writes
 * y HEAD-MAJOR [B][3*H][tokens][dh] (rows m = b*tokens + t, column n -> group n/dh), so that every head's
 * q/k/v block is contiguous for mv_mha_heads_fwd (128-byte pieces at a 3*H*dh stride are served by HBM
 * at about half rate -- tools/ubench/stride_read.hip).  mv_linear_heads_supported() says whether this
 * shape has the path (bf16, dh = 64, M a multiple of tokens, large enough for the 256-row GEMM);
 * otherwise use mv_linear_fwd + mv_mha_fwd. */
int mv_linear_heads_supported(int64_t M, int N, int K, int tokens, int dh, int dtype);
int mv_linear_heads_fwd(const void* x, const void* w, const float* scale, const float* shift, void* y,
                        int64_t M, int N, int K, int tokens, int dh, int dtype, mv_stream_t stream);
int mv_mha_heads_fwd(const void* qkv_head_major, void* out, float* probs, int B, int N, int H, int dh,
                     float scale, int dtype, mv_stream_t stream);

/* _VitBlock (vit.py:139-157) in inference: x = x + proj(attn(norm1(x))); x = x + fc2(gelu(fc1(norm2(x)))).  The LayerNorm
 * between a residual-producing Linear (proj, fc2) and the next Linear (fc1, the next block's qkv) is folded into the two
 * GEMM epilogues -- no LayerNorm launch, no second read of the fp32 rows:
 *     LN(y) . W^T + b  =  rstd * (y . W'^T - mean * colsum(W')) + b',     W' = W . diag(gamma),  b' = b + W . beta
 *   mv_linear_lnout_fwd   y[M][N] = residual + x[M][K] . w[N][K]^T + shift, the residual STREAM kept as two bf16 planes:
 *                         hi = bf16(y), lo = bf16(y - hi) -- the four bytes per value of fp32, ~16 mantissa bits (2^-17 relative per
 *                         store, against the 2^-9 of the operands); the high plane IS the next Linear's operand, so the fold
 *                         costs no extra copy of the rows.  Forms:
 *                           res fp32 rows (res_lo NULL)      -> planes (y, y_lo) + stats     the first block (token rows are fp32)
 *                           res planes (res, res_lo)         -> planes (y, y_lo) + stats
 *                           res planes (res, res_lo)         -> fp32 rows y (y_lo, stats NULL)   the stream leaves the split form
 *                         stats[ceil(N/256)][M][2] fp32 = per row and 256-column piece j (its last one: what is left of N) the pair
 *                         (sum, sum of squared deviations from the piece's own mean) -- merged by the consumer with Chan's
 *                         formula, so no E[x^2] - mean^2 cancellation.
 *   mv_linear_lnin_fwd    y[M][N] bf16 = act(rstd[m] * (x[M][K] . w_folded[N][K]^T - mean[m] * colsum[n]) + shift[n]), x = the
 *                         producer's HIGH plane (un-normalised rows), stats = its table ([ceil(K/256)][M][2]), (mean, rstd) with the
 *                         biased variance and `eps` as eqx.nn.LayerNorm; colsum[n] = sum_k float(w_folded[n][k]) (of the
 *                         bf16-ROUNDED values), shift = b'.  tokens > 0: head-major output as mv_linear_heads_fwd.  K <= 768.
 * The operand is rounded to bf16 BEFORE the mean is removed (the un-fused path rounds LN(y)): the relative error of the two is
 * the same while |mean| <~ std of a row, and grows with |mean| / std beyond -- the host uses the pair for the ViT blocks'
 * residual stream only (switch: no_ln_fold).  Both need the 256 x 256 GEMM tile to be the dispatch's choice for the shape. */
int mv_linear_lnout_supported(int64_t M, int N, int K, int dtype);
int mv_linear_lnout_fwd(const void* x, const void* w, const float* shift, const void* res, const void* res_lo, void* y,
                        void* y_lo, float* stats, int64_t M, int N, int K, int dtype, mv_stream_t stream);
int mv_linear_lnin_supported(int64_t M, int N, int K, int tokens, int dh, int dtype);
int mv_linear_lnin_fwd(const void* x, const float* stats, const void* w_folded, const float* colsum, const float* shift,
                       void* y, int64_t M, int N, int K, float eps, int act, int tokens, int dh, int dtype,
                       mv_stream_t stream);

/* The same attention core with the reference's LIVE attention dropout (vit.py:71, training mode: attn =
 * attn_drop(softmax(...), key)): every probability is kept (and divided by keep_prob) or zeroed by word
 * ((h * N + i) * N + j) of the sample's Threefry-2x32 stream -- jax.random.bernoulli(key, keep_prob,
 * (1, H, N, N)) bit for bit -- before it multiplies V; probs (optional) receives the dropped matrix, which
 * is what the reference returns.  keys: B x 2 uint32 (one key per sample); qkv token-major (head_major = 0,
 * as mv_mha_fwd) or head-major (1, as mv_mha_heads_fwd).  bf16, dh 32 / 64, N <= 256, else MV_E_UNSUPPORTED. */
int mv_mha_dropout_fwd(const void* qkv, int head_major, void* out, float* probs, const uint32_t* keys,
                       float keep_prob, int B, int N, int H, int dh, float scale, int dtype,
                       mv_stream_t stream);

/* _shifted_window_attention core (swin.py:123-250) on the qkv Linear2d output:
 * qkv NHWC [B,Hf,Wf,3*C] -> out NHWC [B,Hf,Wf,C]; cyclic shift, window partition/reverse and
 * the shift mask are folded into addressing; bias fp32 [heads][ws*ws][ws*ws] (table[index]). */
int mv_swin_window_attn_fwd(const void* qkv, const float* bias, void* out, int B, int Hf, int Wf, int C,
                            int heads, int ws_h, int ws_w, int shift_h, int shift_w,
                            int dtype, mv_stream_t stream);

/* The reference's two `_func_dropout` calls inside `_shifted_window_attention` (swin.py:17-20, :227, :233 -- applied in
 * EVERY mode, the function has no inference switch; both draw from the SAME key):
 * mv_swin_window_attn_dropout_fwd: the attention core with the probabilities (num_windows, heads, n, n) of every sample dropped
 * by jax.random.bernoulli(key, keep_prob, that shape) between the softmax and P . V (MFMA path only: bf16, 32 channels per
 * head, <= 64 tokens per window, else MV_E_UNSUPPORTED);
 * mv_dropout_windows_fwd: Dropout of the projection's output, an NHWC map here, in the LOGICAL order (num_windows, n, C) of the
 * shifted, window-partitioned map it has in the reference at that point.  keys: [B][2] uint32 on the device. */
int mv_swin_window_attn_dropout_fwd(const void* qkv, const float* bias, void* out, const void* keys, float keep_prob, int B,
                                    int Hf, int Wf, int C, int heads, int ws_h, int ws_w, int shift_h, int shift_w,
                                    int dtype, mv_stream_t stream);
int mv_dropout_windows_fwd(const void* x, const void* keys, void* y, int B, int Hf, int Wf, int C, int ws_h, int ws_w,
                           int shift_h, int shift_w, float keep_prob, int dtype, mv_stream_t stream);

/* Swin V2's cosine attention (`_shifted_window_attention` with logit_scale, swin.py:144-168; `_ShiftedWindowAttentionV2` :369-522).
 * mv_swin_qk_rnorm_fwd: the reference divides q and k, shaped (nW, heads, n, dh), by jnp.linalg.norm(., ord=2, axis=0) (:161-163):
 * axis 0 is the WINDOWS of one image.  rnorm fp32 [B][2][n][C] (s = 0: q, s = 1: k; n = ws_h * ws_w) =
 * 1 / sqrt(sum over the nW windows w of x_s[w][t][c]^2) on the rolled, partitioned map (the token walk of mv_swin_window_attn_fwd);
 * fp32 accumulation in increasing window order; the value third of qkv is never read.  A map that is not a multiple of the window,
 * or C that is not a whole number of 16-byte chunks: MV_E_UNSUPPORTED.  A zero norm gives inf, as the reference's division does.
 * mv_swin_window_attn_cos_fwd: the attention core with logits (q * rnorm_q) . (k * rnorm_k)^T * logit_mul[h] + bias (:161-173; no
 * dh^-0.5): logit_mul fp32 [heads] = exp(min(logit_scale, log 100)) (:165-167), bias fp32 [heads][n][n] = 16 sigmoid(cpb_mlp(..))
 * gathered on the host (:486-495).  bf16 with 32 channels per head and n <= 64 runs on the MFMA kernel (the scaled q / k fragments
 * are rounded once to bf16); everything else on the one-wave-per-query kernel.  keys != NULL: the reference's attention dropout
 * (:227) as in mv_swin_window_attn_dropout_fwd, MFMA path only, else MV_E_UNSUPPORTED; keys NULL: keep_prob is ignored. */
int mv_swin_qk_rnorm_fwd(const void* qkv, float* rnorm, int B, int Hf, int Wf, int C, int ws_h, int ws_w, int shift_h,
                         int shift_w, int dtype, mv_stream_t stream);
int mv_swin_window_attn_cos_fwd(const void* qkv, const float* rnorm, const float* logit_mul, const float* bias, void* out,
                                const void* keys, float keep_prob, int B, int Hf, int Wf, int C, int heads, int ws_h, int ws_w,
                                int shift_h, int shift_w, int dtype, mv_stream_t stream);

/* The post-norm residual step of `_SwinTransformerBlockV2` (swin.py:629-635: x + norm(branch(x))) and the norm of `_PatchMergingV2`
 * (:83-87, res = NULL):  y[m][:] = res[m][:] + gamma * n(z[m][:]) + beta  over M rows of C; z bf16 / fp32 (z_dtype), res fp32 or
 * NULL, y fp32.  y_lo (lo_dtype, or NULL): the same row rounded once (round-to-nearest-even) -- the operand plane of the next
 * Linear, so the fp32 stream needs no cast launch.  C a whole number of 16-byte chunks of z, at most 512 of them (96 .. 1024 and
 * beyond), else MV_E_UNSUPPORTED. */
int mv_layernorm_add_fwd(const void* z, const float* res, const float* gamma, const float* beta, float* y, void* y_lo, int64_t M,
                         int C, float eps, int z_dtype, int lo_dtype, mv_stream_t stream);

/* _patch_merging_pad (swin.py:23-31): NHWC [B,H,W,C] -> [B,H/2,W/2,4C], channel blocks
 * [x(0::2,0::2) | x(1::2,0::2) | x(0::2,1::2) | x(1::2,1::2)], zero pad odd H/W. */
int mv_patch_merge_gather_nhwc(const void* x, void* y, int B, int H, int W, int C, int dtype, mv_stream_t stream);

/* Swin patch embedding + its LayerNorm in one launch (swin.py:705-711: LayerNorm2d(Conv2d(3, K, kernel 4, stride 4)(x))): x MV_F32
 * NCHW [B][3][H][W] -> y MV_F32 NHWC [B][H/4][W/4][K] (the fp32 residual stream).  w_hi [K][48] bf16 (OIHW flattened), w_lo = the low
 * halves of split-precision weights (hi + lo ~ the fp32 weight) or NULL, bias [K] or NULL.  K = 96 or 128; H, W multiples of 4. */
int mv_patch4_ln_supported(int C, int H, int W, int K, int x_dtype);
int mv_patch4_ln_fwd(const void* x, const void* w_hi, const void* w_lo, const float* bias, const float* gamma, const float* beta,
                     void* y, int B, int C, int H, int W, int K, float eps, int x_dtype, mv_stream_t stream);

/* Swin patch merging's gather + its LayerNorm (swin.py:23-31, 61-65: `norm(_patch_merging_pad(x))`) in one pass: row (b, i, j) of y
 * is the LayerNorm over the 4 C channels [x[2i,2j] | x[2i+1,2j] | x[2i,2j+1] | x[2i+1,2j+1]] of the fp32 NHWC map x; y [B][H/2][W/2][4C]
 * in out_dtype.  H, W even, C % 4 == 0, C <= 384. */
int mv_patch_merge_ln_supported(int H, int W, int C, int x_dtype);
int mv_patch_merge_ln_fwd(const void* x, const float* gamma, const float* beta, void* y, int B, int H, int W, int C, float eps,
                          int x_dtype, int out_dtype, mv_stream_t stream);

/* vit.py:269 row 0 of every image: tokens[b,0,:] = cls[:] + pos[0,:] (fp32 inputs). */
int mv_vit_cls_pos_fwd(const float* cls, const float* pos, void* tokens, int B, int tok_stride, int D,
                       int dtype, mv_stream_t stream);

/* jax.nn.relu / jax.nn.gelu (tanh form) / residual add as standalone ops (unfused call sites) */
int mv_eltwise_fwd(const void* x, void* y, int64_t n, int act, int dtype, mv_stream_t stream);
int mv_add_fwd(const void* a, const void* b, void* y, int64_t n, int act, int dtype, mv_stream_t stream);
/* per-channel affine y = act(x*scale[c] + shift[c]) over rows of C (stand-alone BatchNorm inference) */
int mv_channel_affine_fwd(const void* x, const float* scale, const float* shift, void* y,
                          int64_t rows, int C, int act, int dtype, mv_stream_t stream);
/* The same with the block's identity added before the activation: y = act(x * scale[c] + shift[c] + residual) -- the tail of a residual
 * block whose BatchNorm is in training mode (resnet.py:155-160 / :88-91); C must be a multiple of 8. */
int mv_channel_affine_res_fwd(const void* x, const float* scale, const float* shift, const void* residual, void* y, int64_t rows,
                              int C, int act, int dtype, mv_stream_t stream);

/* layout / dtype plumbing at the user boundary */
int mv_nchw_to_nhwc(const void* x, void* y, int N, int C, int H, int W, int in_dtype, int out_dtype, mv_stream_t stream);
int mv_nhwc_to_nchw(const void* x, void* y, int N, int C, int H, int W, int in_dtype, int out_dtype, mv_stream_t stream);
int mv_cast(const void* x, void* y, int64_t n, int in_dtype, int out_dtype, mv_stream_t stream);

/* ---- backward half of a training step (reference tests/test_grads.py:35-47: eqx.filter_value_and_grad +
 * optax.adam + eqx.apply_updates on the classification models).  fp32 throughout.  The contractions that are a forward
 * contraction on other operands (Linear dgrad / wgrad, the four products of attention's backward) go through mv_linear_fwd on
 * operands transposed with mv_transpose2d_f32 (eqxvision_amd/grad.py); these entries are the gradient kernels with no forward twin. */
/* Conv2d (eqx.nn.Conv2d incl. grouped / depthwise): dx[N,H,W,C] from dy[N,Ho,Wo,K] and w [K][R][S][C/groups]; dw in the same
 * layout from x and dy.  Both run on the fp32 matrix cores (dgrad: groups = 1).  The weight gradient's reduction runs over all
 * N Ho Wo output positions: with scratch on offer (mv_set_scratch, any size from 4096 + 2 x the gradient's bytes up) the positions are split
 * over blocks and the parts added in a fixed order (bit-reproducible); without it one block walks all positions of its tile. */
int mv_conv2d_dgrad_nhwc_f32(const float* dy, const float* w_krsc, float* dx, int N, int H, int W, int C, int K, int R, int S,
                             int sh, int sw, int ph, int pw, int dh, int dw, int groups, mv_stream_t stream);
int mv_conv2d_wgrad_nhwc_f32(const float* x, const float* dy, float* dw_krsc, int N, int H, int W, int C, int K, int R, int S,
                             int sh, int sw, int ph, int pw, int dh, int dw, int groups, mv_stream_t stream);
/* dx = dy * act'(ref), ref = the activation's INPUT: every MV_ACT_* (relu, gelu-tanh, hard_swish, hard_sigmoid, sigmoid, silu). */
int mv_act_bwd_f32(const float* dy, const float* ref, float* dx, int64_t n, int act, mv_stream_t stream);
/* eqx.nn.MaxPool2d backward: dy goes to the first maximum of each window (x = the forward input). */
int mv_maxpool2d_bwd_nhwc_f32(const float* x, const float* dy, float* dx, int N, int H, int W, int C, int kh, int kw, int sh, int sw,
                              int ph, int pw, mv_stream_t stream);
/* AdaptiveAvgPool2d((1,1)) backward: dx[n,h,w,c] = dy[n,c] / (H W). */
int mv_avgpool_global_bwd_nhwc_f32(const float* dy, float* dx, int N, int HW, int C, mv_stream_t stream);
/* Attention backward (vit.py:64-73, the op of mv_mha_fwd with the probabilities kept): dqkv[B,N,3,H,dh] from qkv (same layout),
 * probs[B,H,N,N] and dout[B,N,H*dh]; ds_scratch: B*H*N*N floats owned by the caller (the softmax gradient, written by the first of the
 * two launches and read by the second).  Every sum runs in index order. */
int mv_mha_bwd_f32(const float* qkv, const float* probs, const float* dout, float* ds_scratch, float* dqkv, int B, int N, int H, int dh,
                   float scale, mv_stream_t stream);
/* out[c] = sum over the M rows of a[m,c] * (b ? b[m,c] : 1): bias / beta gradients (b = NULL), gamma gradients (b = x_hat).  From 512
 * rows up it takes 4096 bytes + ceil(M / 256) (<= 512) x C floats of scratch when on offer (mv_set_scratch): rows split over blocks, fixed-order finish. */
int mv_colsum_f32(const float* a, const float* b, float* out, int64_t M, int C, mv_stream_t stream);
/* y = x * s[b, c] (SqueezeExcitation's multiply, DropPath): ds[b, c] = sum over the image's HW positions of g * x; dx is the
 * forward multiply applied to g (mv_channel_scale_nhwc_fwd). */
int mv_channel_scale_bwd_f32(const float* g, const float* x, float* ds, int B, int HW, int C, mv_stream_t stream);
/* BatchNorm gamma gradient when the normalisation used the RUNNING statistics (the reference's training branch; the state is not
 * differentiated): dgamma[c] = (sum dy z - mean[c] sum dy) / sqrt(var[c] + eps), from the two column sums. */
int mv_bn_dgamma_f32(const float* sum_dy_z, const float* sum_dy, const float* mean, const float* var, float eps, float* dgamma, int C,
                     mv_stream_t stream);
/* eqx.experimental.BatchNorm TRAINING branch, input gradient through the batch statistics.  The layer normalises with
 * running' = a * batch + (1 - a) * running (a = 1 on the first call, 1 - momentum afterwards) and the batch mean / variance are
 * differentiable functions of z, so   dz = scale * dy + A[c] + B[c] * z   with scale = gamma * rstd(running'),
 *   B[c] = -(a / n) * scale * rstd^2 * (sum dy z - mean'[c] sum dy),   A[c] = -(a / n) * scale * sum dy - B[c] * batch_mean[c],
 * batch_mean = sum_z / n.  The three column sums are over ALL n rows of the data-parallel batch (summed over ranks by the caller);
 * n = *count when count != NULL (device scalar: ragged shards), else rows. */
int mv_bn_train_dz_coef_f32(const float* sum_dy, const float* sum_dy_z, const float* sum_z, const float* mean, const float* var,
                            const float* scale, const float* count, float rows, float a, float eps, float* A, float* B, int C,
                            mv_stream_t stream);
/* eqx.nn.LayerNorm backward over M rows of C (x = the forward input): dx, and dy_xhat = dy * x_hat (its column sums = dgamma;
 * the column sums of dy = dbeta). */
int mv_layernorm_bwd_f32(const float* x, const float* gamma, const float* dy, float* dx, float* dy_xhat, int64_t M, int C, float eps,
                         mv_stream_t stream);
/* softmax backward for p = softmax(scale * s) row-wise: ds = scale * p * (dp - sum_j dp_j p_j). */
int mv_softmax_bwd_f32(const float* p, const float* dp, float* ds, int64_t rows, int cols, float scale, mv_stream_t stream);
/* optax.softmax_cross_entropy(logits, target).mean() (tests/test_grads.py:41): loss_rows[B], loss_mean[1], dlogits = d mean / d logits. */
int mv_softmax_xent_f32(const float* logits, const float* target, float* loss_rows, float* loss_mean, float* dlogits, int B, int K,
                        mv_stream_t stream);
/* optax.adam (tests/test_grads.py:52): m, v updated in place, update = -lr * (m / bias_corr1) / (sqrt(v / bias_corr2) + eps) with
 * bias_corr = 1 - beta^t computed by the caller; eqx.apply_updates adds `update` to the parameter (mv_add_fwd). */
int mv_adam_step_f32(const float* grad, float* m, float* v, float* update, int64_t n, float lr, float b1, float b2, float eps,
                     float bias_corr1, float bias_corr2, mv_stream_t stream);
/* ---- optimisers over a whole parameter set (csrc/optim.hip).  One record per tensor, all records in ONE device
 * buffer; a 256-thread workgroup owns one chunk of MV_OPTIM_CHUNK elements of one tensor and finds its record by binary search of
 * first_block over its block index (first_block[0] = 0, first_block[i + 1] = first_block[i] + ceil(n[i] / MV_OPTIM_CHUNK),
 * total_blocks = the sum).  param / m / v may be NULL where the rule does not use them; grad, out and n > 0 are required.  A
 * tensor whose pointers are all 16-byte aligned is streamed as float4 (scalar tail for n % 4), any other element by element.  No
 * atomics; out may alias nothing else of its record.  The records are trusted: the caller builds them from live allocations. */
#define MV_OPTIM_CHUNK 4096
typedef struct mv_optim_tensor {
    const float* grad;
    const float* param;
    float* m;
    float* v;
    float* out;
    int64_t n;
    int64_t first_block;
} mv_optim_tensor;                               /* 56 bytes, no padding */
enum { MV_OPT_SGD = 0, MV_OPT_ADAMW = 1, MV_OPT_APPLY = 2, MV_OPT_EMA = 3 };
/* Sum of squares of every grad of the set, and optax.clip_by_global_norm's factor.  Two launches: every workgroup writes the sum
 * of its chunk to partial[block] (total_blocks floats; per lane in element order, a fixed butterfly over the wave, the four waves
 * in order through LDS), then one workgroup adds the partials (thread t takes t, t + 256, ... in order, then the same tree) and
 * writes out2[0] = sum, out2[1] = (sqrt(sum) < max_norm ? 1 : max_norm / sqrt(sum)).  The order is fixed: same bits every run. */
int mv_optim_sqnorm_f32(const mv_optim_tensor* recs, int n_tensors, int64_t total_blocks, float* partial, float* out2,
                        float max_norm, mv_stream_t stream);
/* One launch over all tensors.  g = grad * scale[1] when scale != NULL (the out2 of mv_optim_sqnorm_f32), else grad.
 *   MV_OPT_SGD   (optax.sgd / trace): m == NULL: out = -lr g.  Else m = g + b1 m (b1 = the momentum), out = -lr m, or with
 *                nesterov != 0 out = -lr (g + b1 m).
 *   MV_OPT_ADAMW (optax.adamw): m = b1 m + one_minus_b1 g, v = b2 v + one_minus_b2 g^2,
 *                out = -lr ((m / bias_corr1) / (sqrt(v / bias_corr2) + eps) + weight_decay param); param may be NULL when
 *                weight_decay == 0.  one_minus_b* and bias_corr* = 1 - b*^t come from the caller (rounded once from float64).
 *   MV_OPT_APPLY (eqx.apply_updates): out = param + grad.
 *   MV_OPT_EMA   (torchvision's ExponentialMovingAverage): out = fadd(fmul(b1, out), fmul(one_minus_b1, grad)) -- out is the
 *                average, read and written; grad the parameter; b1 the decay -- or, with nesterov != 0, out = grad (the first
 *                update after init copies).  Two rounded products and one rounded sum, no contraction; scale is not applied. */
int mv_optim_step_f32(const mv_optim_tensor* recs, int n_tensors, int64_t total_blocks, int kind, int nesterov, float lr, float b1,
                      float b2, float one_minus_b1, float one_minus_b2, float eps, float weight_decay, float bias_corr1,
                      float bias_corr2, const float* scale, mv_stream_t stream);
/* Backward of mv_swin_window_attn_fwd (swin.py:123-250), fp32: dqkv[B,Hf,Wf,3C] from qkv, the relative-position bias
 * [heads][n][n] and dout[B,Hf,Wf,C]; g_windows [B * windows][heads][n * n] receives the gradient w.r.t. the attention logits of
 * every window (its column sum over the windows = the bias gradient).  Windows of <= 64 tokens. */
int mv_swin_window_attn_bwd_f32(const float* qkv, const float* bias, const float* dout, float* dqkv, float* g_windows, int B, int Hf,
                                int Wf, int C, int heads, int ws_h, int ws_w, int shift_h, int shift_w, mv_stream_t stream);
/* out[t][c] = sum of src[m][c] over the rows m with index[m] == t (t < T): the gradient of a table gathered by `index`
 * (swin.py:34-43: relative_position_bias_table[relative_position_index]). */
int mv_scatter_rows_sum_f32(const float* src, const int* index, float* out, int M, int C, int T, mv_stream_t stream);
/* Backward of mv_patch_merge_gather_nhwc (swin.py:23-31) for even H, W: dx[B,H,W,C] from dy[B,H/2,W/2,4C]. */
int mv_patch_merge_gather_bwd_f32(const float* dy, float* dx, int B, int H, int W, int C, mv_stream_t stream);
/* Adjoint of mv_resize_bilinear_nhwc_fwd for H >= h, W >= w (half-pixel centres, edge clamp: jax.image.resize "bilinear"; down-sampling
 * returns MV_E_INVALID): dx[N,h,w,C] from dy, which is [N,C,H,W] when dy_nchw (the out_nchw = 1 form the segmentation models return),
 * else [N,H,W,C].  Gather form: every dx element sums its own footprint of dy in a fixed order -- one launch, no atomics, bit-reproducible. */
int mv_resize_bilinear_bwd_nhwc_f32(const float* dy, float* dx, int N, int h, int w, int C, int H, int W, int dy_nchw,
                                    mv_stream_t stream);
/* optax.softmax_cross_entropy_with_integer_labels over the class axis of NCHW logits [B, C, HW]: labels int32 [B, HW]; where uint8
 * [B, HW] or NULL (every pixel counts).  loss[B, HW] per pixel (0 where masked), dlogits[B, C, HW] = d sum(loss) / d logits (0 where
 * masked; the caller applies the 1 / n of a mean), sums[2] = {sum of loss, number of counted pixels}, added in a fixed order.
 * A label outside [0, C) on a counted pixel is never used as an index; it raises bit 1 of the device status word (mv_device_status). */
int mv_softmax_xent_map_f32(const float* logits, const int32_t* labels, const uint8_t* where, float* loss, float* dlogits, float* sums,
                            int B, int C, int64_t HW, mv_stream_t stream);
/* y[C][R] = x[R][C]^T, rows of x x_row_stride elements apart (0 = dense). */
int mv_transpose2d_f32(const float* x, float* y, int R, int C, int64_t x_row_stride, mv_stream_t stream);

/* ---- mixed-precision Linear for the training step (filter_value_and_grad(..., matmul_dtype="bf16"); eqx.nn.Linear under vmap:
 * vit.py:64,74; mlps.py:60-64; swin.py).  Every tensor is fp32 in memory.  r(.) rounds an operand element to bf16, round-to-nearest-
 * even, on its way into LDS; products are accumulated in fp32 on v_mfma_f32_32x32x16_bf16 and the result is stored as fp32.  Any
 * M, N, K >= 1 (N, K <= 2^21); no transposed copy of an operand is made: the operands whose reduction runs along their rows are
 * read from LDS with the transposed read.  16-byte loads where base and row pitch are 16-byte aligned, 4-byte loads otherwise.
 *   fwd:    y[M,N]  = r(x[M,K]) . r(w[N,K])^T + bias[n]   (bias may be NULL; it is added in fp32, NOT rounded)
 *   dgrad:  dx[M,K] = r(g[M,N]) . r(w[N,K])               (reduction over N)
 *   wgrad:  dw[N,K] = r(g[M,N])^T . r(x[M,K])             (reduction over M).  With scratch on offer (mv_set_scratch: 4096 bytes + at
 *           least 2 x the gradient's bytes) the rows are split over up to 64 parts of at least 256 rows, which are added in index order
 *           (bit-reproducible; the first 4096 bytes of the offer stay zero); without it one block walks all of M for its tile (same
 *           result to within fp32 summation order).  mv_last_kernel tells the two forms apart. */
int mv_linear_mp_fwd(const float* x, const float* w, const float* bias, float* y, int64_t M, int N, int K, mv_stream_t stream);
int mv_linear_mp_dgrad(const float* g, const float* w, float* dx, int64_t M, int N, int K, mv_stream_t stream);
int mv_linear_mp_wgrad(const float* g, const float* x, float* dw, int64_t M, int N, int K, mv_stream_t stream);

/* ---- mixed-precision Conv2d, groups == 1, for the training step (filter_value_and_grad(..., conv_dtype="bf16"); eqx.nn.Conv2d).
 * Implicit GEMMs, no im2col buffer.  Maps are NHWC fp32, filters KRSC fp32 (w[k][r][s][c]); every tensor is fp32 in memory.  r(.)
 * rounds an operand element to bf16, round-to-nearest-even, on its way into LDS; products are accumulated in fp32 on
 * v_mfma_f32_32x32x16_bf16 and the result is stored as fp32.  Any R, S and any stride / padding / dilation (h and w independent).
 * Ho = (H + 2 ph - dh (R - 1) - 1) / sh + 1, Wo likewise; an empty output is MV_E_INVALID.
 *   fwd:    y[n,ho,wo,k]  = sum over r, s, c of r(x[n, ho sh - ph + r dh, wo sw - pw + s dw, c]) r(w[k,r,s,c]) + bias[k]
 *           (padding reads as zeros; bias may be NULL; it is added in fp32, NOT rounded)
 *   dgrad:  dx[n,hi,wi,c] = sum over k and over the taps (r, s) for which sh divides hi + ph - r dh and sw divides wi + pw - s dw with
 *           both quotients (ho, wo) inside the output map, of r(dy[n,ho,wo,k]) r(w[k,r,s,c]); every dx element is written
 *   wgrad:  dw[k,r,s,c]   = sum over the output positions (n, ho, wo) of r(dy[n,ho,wo,k]) r(x[n, ho sh - ph + r dh, wo sw - pw + s dw, c]).
 *           With scratch on offer (mv_set_scratch: 4096 bytes + at least 2 x the gradient's bytes) the positions are split over up to
 *           64 parts of at least 256 positions, which are added in index order (bit-reproducible; the first 4096 bytes of the offer
 *           stay zero); without it, or with room for fewer than two parts, one block walks all positions for its tile and writes dw
 *           directly.  mv_last_kernel tells the two forms apart (conv_mp_wgrad_bf16 / conv_mp_wgrad_split_bf16).
 * Limits: C, K and R S C at most 2^21; x and y / dy at most 2^29 - 4 elements each (the gathered map is addressed with 32-bit byte
 * offsets from its base): a larger map is refused with MV_E_UNSUPPORTED, never wrapped.  16-byte loads where base and channel count
 * allow (16-byte aligned base, C resp. K a multiple of 4), 4-byte loads otherwise. */
int mv_conv2d_mp_fwd(const float* x, const float* w_krsc, const float* bias, float* y, int N, int H, int W, int C, int K, int R, int S,
                     int sh, int sw, int ph, int pw, int dh, int dw, mv_stream_t stream);
int mv_conv2d_mp_dgrad(const float* dy, const float* w_krsc, float* dx, int N, int H, int W, int C, int K, int R, int S, int sh, int sw,
                       int ph, int pw, int dh, int dw, mv_stream_t stream);
int mv_conv2d_mp_wgrad(const float* x, const float* dy, float* dw_krsc, int N, int H, int W, int C, int K, int R, int S, int sh, int sw,
                       int ph, int pw, int dh, int dw, mv_stream_t stream);

/* ---- mixed-precision attention core for the training step (filter_value_and_grad(..., attn_dtype="bf16"); vit.py:65-73, the op of
 * mv_mha_fwd / mv_mha_bwd_f32).  qkv and dqkv are fp32 token-major [B, N, 3, H, dh]; out and dout fp32 [B, N, H*dh]; lse fp32
 * [B, H, N]; probs fp32 [B, H, N, N] or NULL.  r(.) rounds an element to bf16, round-to-nearest-even, on its way into LDS or
 * registers; products accumulate in fp32 on v_mfma_f32_32x32x16_bf16; nothing in memory changes type.
 *   fwd:  s_ij = sum_d r(q_id) r(k_jd);  pe_ij = exp(scale s_ij - max_j scale s_ij);  Z_i = sum_j pe_ij (pe un-rounded)
 *         out_i = (sum_j r(pe_ij) r(v_j)) / Z_i;  lse_i = max_j scale s_ij + log Z_i;  probs_ij = pe_ij / Z_i, written only when
 *         probs != NULL (out and lse do not depend on it)
 *   bwd:  from qkv, out, dout and lse, the probabilities recomputed: p_ij = exp(scale s_ij - lse_i);  delta_i = sum_d dout_id out_id
 *         (fp32, un-rounded);  dp_ij = sum_d r(dout_id) r(v_jd);  ds_ij = scale p_ij (dp_ij - delta_i);  dV_j = sum_i r(p_ij) r(dout_i);
 *         dQ_i = sum_j r(ds_ij) r(k_j);  dK_j = sum_i r(ds_ij) r(q_i).  No atomics, one summation order: two runs give the same bits.
 * mv_mha_mp_supported: dh 32 / 64 and 1 <= N <= 256.  Anything else is MV_E_UNSUPPORTED, a NULL or not 16-byte aligned pointer or
 * scale <= 0 is MV_E_INVALID; either is returned before any HIP call and leaves the destinations untouched. */
int mv_mha_mp_supported(int N, int dh);
int mv_mha_mp_fwd(const float* qkv, float* out, float* lse, float* probs, int B, int N, int H, int dh, float scale, mv_stream_t stream);
int mv_mha_mp_bwd(const float* qkv, const float* out, const float* dout, const float* lse, float* dqkv, int B, int N, int H, int dh,
                  float scale, mv_stream_t stream);

/* ---- mixed-precision Swin shifted-window attention for the training step (the same keyword, attn_dtype="bf16"; swin.py:123-250, the op
 * of mv_swin_window_attn_fwd / mv_swin_window_attn_bwd_f32).  qkv and dqkv are fp32 NHWC [B, Hf, Wf, 3C], columns [q|k|v][head][dh];
 * out and dout fp32 [B, Hf, Wf, C]; bias fp32 [heads, n, n] (n = ws_h * ws_w); lse fp32 [B * nW, heads, n] in window order;
 * dbias_parts fp32 [P, heads, n, n] with P = mv_swin_attn_mp_bwd_parts(...), or NULL.  r(.) as above; roll, partition and shift mask
 * are index arithmetic, and the shift of an axis whose window covers the map is dropped.
 *   fwd:  l_ij = scale sum_d r(q_id) r(k_jd) + bias[h][i][j] + (shifted and region_i != region_j ? -100 : 0)   (q is NOT pre-scaled)
 *         pe_ij = exp(l_ij - max_j l_ij);  Z_i = sum_j pe_ij (un-rounded);  out_i = (sum_j r(pe_ij) r(v_j)) / Z_i;  lse_i = max_j l_ij + log Z_i
 *   bwd:  p_ij = exp(l_ij - lse_i) recomputed from qkv, bias, mask and the given lse;  delta_i = sum_d dout_id out_id (fp32, un-rounded)
 *         dp_ij = sum_d r(dout_id) r(v_jd);  g_ij = p_ij (dp_ij - delta_i);  dV_j = sum_i r(p_ij) r(dout_i)
 *         dQ_i = scale sum_j r(g_ij) r(k_j);  dK_j = scale sum_i r(g_ij) r(q_i)
 *         dbias_parts[p][h][i][j] = the sum of the un-rounded g_ij over the (image, window) pairs p, p + P, p + 2 P, .. in that order:
 *         every element of every part is written (zeros where a part has no pair); the bias gradient is the sum of the parts
 *         (mv_colsum_f32 over P rows).  With dbias_parts == NULL nothing is accumulated or written.  No atomics: two runs, same bits.
 * P depends on the arguments of mv_swin_attn_mp_bwd_parts alone and is at most 2048 / heads (at least 1), whatever B is.
 * mv_swin_attn_mp_supported: dh 32 / 64 and 1 <= n <= 64.  Anything else, or B * nW * heads >= 2^31, is MV_E_UNSUPPORTED; a NULL or
 * not 16-byte aligned pointer, a window that does not divide the map, a shift outside the window or scale <= 0 is MV_E_INVALID;
 * either is returned before any HIP call and leaves the destinations untouched. */
int mv_swin_attn_mp_supported(int n_tokens, int dh);
int mv_swin_attn_mp_bwd_parts(int B, int Hf, int Wf, int heads, int ws_h, int ws_w);
int mv_swin_attn_mp_fwd(const float* qkv, const float* bias, float* out, float* lse, int B, int Hf, int Wf, int C, int heads, int ws_h,
                        int ws_w, int shift_h, int shift_w, float scale, mv_stream_t stream);
int mv_swin_attn_mp_bwd(const float* qkv, const float* bias, const float* out, const float* dout, const float* lse, float* dqkv,
                        float* dbias_parts, int B, int Hf, int Wf, int C, int heads, int ws_h, int ws_w, int shift_h, int shift_w,
                        float scale, mv_stream_t stream);

/* hipGraph capture of a whole forward (replaces the reference's eqx.filter_jit executable) */
int mv_graph_begin_capture(mv_stream_t stream);
int mv_graph_end_capture(mv_stream_t stream, void** graph_exec);
int mv_graph_launch(void* graph_exec, mv_stream_t stream);
int mv_graph_destroy(void* graph_exec);

/* Training-mode Dropout (eqx.nn.Dropout with inference = False: alexnet.py:63-68, vit.py:39-53, mlps.py:43-52 before
 * tree_inference): y = where(bernoulli(key_b, keep_prob, x_b.shape), x_b / keep_prob, 0) for every sample b, keys [B][2]
 * uint32 on the device (one jax.random key per sample, as under vmap).  The mask is JAX's bit stream: Threefry-2x32 words in
 * jax.random's counter layout, word i for element i of the LOGICAL single-sample array in row-major order -- the reference's
 * (C,H,W) when chw_logical != 0 (x is NHWC [B][per_sample / C][C] here), else the physical order ((N,D) rows, (D,) vectors). */
int mv_dropout_fwd(const void* x, const void* keys, void* y, int B, int64_t per_sample, int C, int chw_logical, float keep_prob,
                   int dtype, mv_stream_t stream);

/* jax.random.split(key, num) for R keys at once, on the device (the reference derives one key per TOKEN for the vmapped
 * transformer MLP, vit.py:155: R = batch * tokens keys per block is host work worth a launch): keys [R][2] uint32 ->
 * out [R][num][2] (child_major = 0: the children of a key together, e.g. the per-token keys of every sample) or [num][R][2]
 * (child_major = 1: what a vmapped split returns, child i of every key contiguous). */
int mv_prng_split(const void* keys, void* out, int64_t R, int num, int child_major, mv_stream_t stream);

/* DropPath's draws (drop_path.py:51-61, training mode) as the scale mv_channel_scale_nhwc_fwd multiplies by: out [B][C] =
 * bernoulli(key_b, keep_prob) / keep_prob for the whole sample (local = 0, mode "global") or bernoulli(key_b, keep_prob, (C,))[c] /
 * keep_prob (local = 1, mode "local": one draw per entry of the sample's first axis), in `dtype`. */
int mv_drop_path_noise(const void* keys, void* out, int B, int C, int local, float keep_prob, int dtype, mv_stream_t stream);

/* Per-channel batch moments of rows x[rows][C] (an NHWC map or a row matrix): the statistics of eqx.experimental.BatchNorm's
 * TRAINING branch (reference resnet.py:132-136 / :252 / :301 with the model not in inference mode):
 *   out[c] = sum over rows of (x[r][c] - shift[c])        (squared = 0; shift may be NULL)
 *   out[c] = sum over rows of (x[r][c] - shift[c])^2      (squared = 1)
 * Two passes like the reference (mean, then the mean of squared deviations from the cross-replica mean); the caller divides by
 * the global row count after mv_allreduce_sum_f32.  workspace: mv_channel_moments_ws(C) floats.  Deterministic summation order. */
int mv_channel_moments_ws(int C);
int mv_channel_moments_supported(int64_t rows, int C, int dtype);
int mv_channel_moments_fwd(const void* x, const float* shift, float* out, float* workspace, int64_t rows, int C, int squared,
                           int dtype, mv_stream_t stream);
/* The rest of the training-mode BatchNorm update on the device, so that a step has no host round trip: mean = sum / n after the
 * first pass (n: the global row count, from the host, or -- ragged shards -- the all-reduced count on the device); after the second:
 * var = sqdev / n, running statistics in place (first call: = batch; else (1 - momentum) * batch + momentum * running, momentum 0.99
 * in the reference), and the scale / shift the normalisation applies (mv_channel_affine_fwd): weight / sqrt(running_var + eps),
 * bias - running_mean * scale -- the UPDATED running statistics, as eqx.experimental.BatchNorm does. */
/* Steady state (running statistics exist): ONE pass and ONE all-reduce of 2 x C floats per layer.  Both moments are taken about the
 * running mean of the previous steps -- the same on every rank, so the ranks' sums add up, and within a fraction of sigma of the batch
 * mean, so var = S2 / n - (S1 / n)^2 loses nothing: out[0:C] = sum (x - shift), out[C:2C] = sum (x - shift)^2 (workspace:
 * 2 * mv_channel_moments_ws(C) floats); mv_bn_ema_fold1_fwd then does what mv_bn_mean_fwd + mv_bn_ema_fold_fwd do for the two-pass
 * form (which the first step of a BatchNorm, with no running statistics yet, still takes -- the reference's literal order). */
int mv_channel_moments2_fwd(const void* x, const float* shift, float* out, float* workspace, int64_t rows, int C, int dtype,
                            mv_stream_t stream);
int mv_bn_ema_fold1_fwd(const float* sums, const float* count_dev, float count_host, float* run_mean, float* run_var,
                        const float* weight, const float* bias, float* scale, float* shift, float momentum, float eps, int C,
                        mv_stream_t stream);
int mv_bn_mean_fwd(const float* sum, const float* count_dev, float count_host, float* mean, int C, mv_stream_t stream);
int mv_bn_ema_fold_fwd(const float* sqdev, const float* mean, const float* count_dev, float count_host, float* run_mean,
                       float* run_var, const float* weight, const float* bias, float* scale, float* shift, float momentum, float eps,
                       int first_time, int C, mv_stream_t stream);

/* The path's one collective: the batch axis of `jax.vmap(net, axis_name="batch")(images)` (README.md:37-40)
 * shards over the GPUs of a node, one process per GPU; rank r runs images[r*B/W:(r+1)*B/W] and ONE all-gather of the fp32 logits
 * rebuilds the (B, classes) array the single-device vmap returns.  RCCL over xGMI (librccl is dlopen'ed by the first call;
 * $EQV_RCCL_LIB overrides the search).  Bootstrap: rank 0 calls mv_comm_unique_id and ships the MV_COMM_ID_BYTES bytes to
 * the other ranks out of band (the Python host uses a torch.distributed gloo store); every rank then calls mv_comm_init
 * with its HIP device already selected.  mv_allgather is enqueued on `stream` like every other call: recv[r*bytes : (r+1)*bytes]
 * = rank r's send buffer.  One communicator per process. */
#define MV_COMM_ID_BYTES 128
int mv_comm_unique_id(void* out, size_t out_bytes);
int mv_comm_init(int rank, int nranks, const void* unique_id);
int mv_comm_size(void); /* 0 = no communicator */
int mv_comm_rank(void);
int mv_allgather(const void* send, void* recv, size_t bytes_per_rank, mv_stream_t stream);
int mv_allreduce_sum_f32(void* buf, size_t count, mv_stream_t stream);   /* in place, sum over ranks (training-mode BatchNorm moments) */
int mv_comm_destroy(void);

/* HIP-event timing helpers on the caller's stream (bench.py's live roofline measurement) */
int mv_event_create(void** ev);
int mv_event_record(void* ev, mv_stream_t stream);
int mv_event_elapsed_ms(void* start, void* stop, float* ms); /* synchronises on stop */
int mv_event_destroy(void* ev);

#ifdef __cplusplus
}
#endif
#endif /* EQXVISION_AMD_H */
