// Decode GEMV entry points: SwiGLU (gate|up with the RMSNorm prologue) and the 16-bit-input
// GEMV (o_proj / down_proj, optional residual accumulate).  Kernels: gemv_kernel.h.
#include "gemv_kernel.h"

CAKE_API int cake_swiglu(int dt, const float* resid, const void* norm_w, float eps,
                         const void* wg, const void* wu, int K, int I, void* act,
                         hipStream_t st) {
  return launch_swiglu<W16>(dt, resid, norm_w, eps, {(const uint16_t*)wg}, {(const uint16_t*)wu},
                            K, I, act, st);
}

CAKE_API int cake_gemv_x16(int dt, const void* x, const void* w, int K, int N, float* out,
                           int accumulate, hipStream_t st) {
  return launch_x16<W16>(dt, x, {(const uint16_t*)w}, K, N, out, accumulate, st);
}
