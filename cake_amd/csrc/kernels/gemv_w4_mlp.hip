// MXFP4 weight-only decode entry point: SwiGLU (gate|up with the RMSNorm prologue),
// cake_swiglu (gemv_mlp.hip) over the format of gemv_w4_kernel.h.
#include "gemv_w4_kernel.h"

CAKE_API int cake_swiglu_w4(int dt, const float* resid, const void* norm_w, float eps,
                            const void* wg, const void* wu, const void* eg, const void* eu,
                            int K, int I, void* act, hipStream_t st) {
  return launch_swiglu<W4>(dt, resid, norm_w, eps, {(const uint8_t*)wg, (const uint8_t*)eg},
                           {(const uint8_t*)wu, (const uint8_t*)eu}, K, I, act, st);
}
