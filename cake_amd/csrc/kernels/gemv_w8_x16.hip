// FP8 (e4m3fn) weight-only decode launcher: the 16-bit-input GEMV (o_proj / down_proj,
// optional residual accumulate).  cake_gemv_x16 (gemv_mlp.hip) with byte weights and a
// row-scale vector.  Kernels: gemv_w8_kernel.h.
#include "gemv_w8_kernel.h"

CAKE_API int cake_gemv_x16_w8(int dt, const void* x, const void* w, const float* scale, int K,
                              int N, float* out, int accumulate, hipStream_t st) {
  if (K < 16 || K % 16 || N < 1) return (int)hipErrorInvalidValue;
  const size_t lds = (size_t)K * 2;
  const GemvTune t = g_tune_w8[kX16W8];
  const int g = grid_for((N + 1) / 2, t.MB);
  if (accumulate) {
    DISPATCH_DT(dt, DISPATCH_W8_TUNE(t, K, CAKE_NX_X16(K, hipLaunchKernelGGL((gemv_x16_w8_kernel<DT, U, PF, NX, true>),
                                                          dim3(g), dim3(kGemvThreads), lds, st,
                                                          (const uint16_t*)x, (const uint8_t*)w,
                                                          scale, K, N, out))));
  } else {
    DISPATCH_DT(dt, DISPATCH_W8_TUNE(t, K, CAKE_NX_X16(K, hipLaunchKernelGGL((gemv_x16_w8_kernel<DT, U, PF, NX, false>),
                                                          dim3(g), dim3(kGemvThreads), lds, st,
                                                          (const uint16_t*)x, (const uint8_t*)w,
                                                          scale, K, N, out))));
  }
  return (int)hipGetLastError();
}
