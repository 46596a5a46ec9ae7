// FP8 (e4m3fn) weight-only decode launcher: SwiGLU (gate|up with the RMSNorm prologue).
// cake_swiglu (gemv_mlp.hip) with byte weights and a row-scale vector for gate and for up.
// Kernels: gemv_w8_kernel.h.
#include "gemv_w8_kernel.h"

CAKE_API int cake_swiglu_w8(int dt, const float* resid, const void* norm_w, float eps,
                            const void* wg, const void* wu, const float* sg, const float* su,
                            int K, int I, void* act, hipStream_t st) {
  if (K < 16 || K % 16 || I < 1) return (int)hipErrorInvalidValue;
  const size_t lds = x32_lds_bytes(K);
  const GemvTune t = g_tune_w8[kSwigluW8];
  // at least one block per 28 rows, as cake_swiglu
  const int mb = t.MB > (I + 27) / 28 ? t.MB : (I + 27) / 28;
  DISPATCH_DT(dt, DISPATCH_W8_TUNE(t, K, CAKE_NX_NORM(K, hipLaunchKernelGGL((swiglu_w8_kernel<DT, U, PF, NX>),
                                                         dim3(grid_for(I, mb)), dim3(kGemvThreads),
                                                         lds, st, resid, (const uint16_t*)norm_w, eps,
                                                         (const uint8_t*)wg, (const uint8_t*)wu, sg,
                                                         su, K, I, (uint16_t*)act))));
  return (int)hipGetLastError();
}
