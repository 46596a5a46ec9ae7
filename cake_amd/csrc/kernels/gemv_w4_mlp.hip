// MXFP4 weight-only decode launcher: SwiGLU (gate|up with the RMSNorm prologue).
// cake_swiglu (gemv_mlp.hip) with packed 4-bit weights and block-scale bytes for gate and
// for up.  Kernels: gemv_w4_kernel.h.
#include "gemv_w4_kernel.h"

CAKE_API int cake_swiglu_w4(int dt, const float* resid, const void* norm_w, float eps,
                            const void* wg, const void* wu, const void* eg, const void* eu,
                            int K, int I, void* act, hipStream_t st) {
  if (K < 32 || K % 32 || I < 1) return (int)hipErrorInvalidValue;
  const size_t lds = x32_lds_bytes4(K);
  const GemvTune t = g_tune_w4[kSwigluW4];
  // at least one block per 28 rows, as cake_swiglu
  const int mb = t.MB > (I + 27) / 28 ? t.MB : (I + 27) / 28;
  DISPATCH_DT(dt, DISPATCH_W4_TUNE(t, K, CAKE_NX_NORM(K, hipLaunchKernelGGL((swiglu_w4_kernel<DT, U, PF, NX>),
                                                         dim3(grid_for(I, mb)), dim3(kGemvThreads),
                                                         lds, st, resid, (const uint16_t*)norm_w, eps,
                                                         (const uint8_t*)wg, (const uint8_t*)wu,
                                                         (const uint8_t*)eg, (const uint8_t*)eu, K, I,
                                                         (uint16_t*)act))));
  return (int)hipGetLastError();
}
