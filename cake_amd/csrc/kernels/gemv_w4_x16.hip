// MXFP4 weight-only decode launcher: the 16-bit-input GEMV (o_proj / down_proj, optional
// residual accumulate).  cake_gemv_x16 (gemv_mlp.hip) with packed 4-bit weights and their
// block-scale bytes.  Kernels: gemv_w4_kernel.h.
#include "gemv_w4_kernel.h"

CAKE_API int cake_gemv_x16_w4(int dt, const void* x, const void* w, const void* e8, int K, int N,
                              float* out, int accumulate, hipStream_t st) {
  if (K < 32 || K % 32 || N < 1) return (int)hipErrorInvalidValue;
  const size_t lds = x16_lds_bytes4(K);
  const GemvTune t = g_tune_w4[kX16W4];
  const int g = grid_for((N + 1) / 2, t.MB);
  if (accumulate) {
    DISPATCH_DT(dt, DISPATCH_W4_TUNE(t, K, CAKE_NX_X16(K, hipLaunchKernelGGL((gemv_x16_w4_kernel<DT, U, PF, NX, true>),
                                                          dim3(g), dim3(kGemvThreads), lds, st,
                                                          (const uint16_t*)x, (const uint8_t*)w,
                                                          (const uint8_t*)e8, K, N, out))));
  } else {
    DISPATCH_DT(dt, DISPATCH_W4_TUNE(t, K, CAKE_NX_X16(K, hipLaunchKernelGGL((gemv_x16_w4_kernel<DT, U, PF, NX, false>),
                                                          dim3(g), dim3(kGemvThreads), lds, st,
                                                          (const uint16_t*)x, (const uint8_t*)w,
                                                          (const uint8_t*)e8, K, N, out))));
  }
  return (int)hipGetLastError();
}
