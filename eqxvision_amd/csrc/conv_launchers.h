// The launchers only the routing entries of conv_fallback.hip call (mv_conv2d_*, mv_linear*, mv_conv1x1_chain*, mv_conv1x1_dual*):
// included by conv_fallback.hip and by the files that define them, nowhere else.
#pragma once
#include "common.h"

namespace mv {

// igemm.hip: every route of route_conv but Kern::generic
int igemm_launch(const void* x, const void* w, const float* scale, const float* shift, const void* residual, void* y,
                 const ConvShape& s, Route r, hipStream_t stream);
int skinny_f32_launch(const void* x, const void* w, const float* scale, const float* shift, void* y, long long M, int C, int K,
                      int act, hipStream_t stream);
int stem_supported(int C, int K, int R, int S, int x_dtype, int out_dtype);
int stem_launch(const void* x, const void* w, const float* scale, const float* shift, void* y, int N, int C,
                int H, int W, int K, int R, int S, int sh, int sw, int ph, int pw, int act, int x_dtype,
                int out_dtype, int tok_stride, int tok_offset, const float* pos, hipStream_t stream,
                const void* w_lo = nullptr);   // w_lo: low halves of split-precision weights (generic kernel only)
int igemm2_dual_launch(const void* x, const void* x2, const void* w, const float* scale, const float* shift, void* y, int N,
                       int Ho, int Wo, int C1, int H2, int W2, int C2, int s2, int K, int act, int tile, hipStream_t st);   // tile: 2 = 256x128, 3 = 256x256
int igemm8_dual_launch(const void* x, const void* x2, const void* w, const float* scale, const float* shift,
                       const void* residual, void* y, int N, int Ho, int Wo, int C1, int H2, int W2, int C2, int s2, int K,
                       int act, int out_dtype, int tile, hipStream_t st);
int chain1x1_supported(long long M, int C, int K, int N2, int dtype);
int chain1x1_launch(const void* x, const void* w3, const float* scale3, const float* shift3, const void* residual, void* y,
                    const void* w1, const float* scale1, const float* shift1, void* t1, long long M, int N2, hipStream_t st);
int chain1x1_dual_supported(long long M, int C1, int C2, int K, int N2, int dtype);
int chain1x1_dual_launch(const void* x, const void* x2, const void* wcat, const float* scale3, const float* shift3, void* y,
                         const void* w1, const float* scale1, const float* shift1, void* t1, long long M, hipStream_t st);
int chain_stream_supported(long long M, int C, int K, int N2, int dtype);
int chain_stream_launch(const void* x, const void* w3, const float* scale3, const float* shift3, const void* residual, void* y,
                        const void* w1, const float* scale1, const float* shift1, void* t1, long long M, hipStream_t st);
int chain_res_supported(long long N, int H, int W, int C, int K, int N2, int sub, int dtype);
int chain_res_launch(const void* t2, const void* residual, const void* wfrag, const void* shifts, void* y, void* t1, int N, int H, int W,
                     int sub, hipStream_t st);
int chain_l2_res_supported(long long N, int H, int W, int C, int K, int N2, int sub, int dtype);
int chain_l2_res_launch(const void* t2, const void* residual, const void* wfrag, const void* shifts, void* y, void* t1, int N, int H,
                        int W, int N2, int sub, hipStream_t st);
int chain_l2_dual_supported(long long M, int C1, int C2, int K, int N2, int dtype);
int chain_l2_dual_launch(const void* t2, const void* x, const void* wfrag, const void* shifts, void* y, void* t1, long long M,
                         hipStream_t st);

}  // namespace mv
