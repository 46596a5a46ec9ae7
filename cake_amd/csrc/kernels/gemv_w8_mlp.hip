// FP8 (e4m3fn) weight-only decode entry point: SwiGLU (gate|up with the RMSNorm prologue),
// cake_swiglu (gemv_mlp.hip) over the format of gemv_w8_kernel.h.
#include "gemv_w8_kernel.h"

CAKE_API int cake_swiglu_w8(int dt, const float* resid, const void* norm_w, float eps,
                            const void* wg, const void* wu, const float* sg, const float* su,
                            int K, int I, void* act, hipStream_t st) {
  return launch_swiglu<W8>(dt, resid, norm_w, eps, {(const uint8_t*)wg, sg},
                           {(const uint8_t*)wu, su}, K, I, act, st);
}
