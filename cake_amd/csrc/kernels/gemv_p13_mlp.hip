// P13 (lossless 13-bit bf16) decode entry points: SwiGLU (gate | up with the RMSNorm prologue)
// and the 16-bit-input GEMV (o_proj / down_proj, optional residual accumulate): cake_swiglu
// and cake_gemv_x16 (gemv_mlp.hip) over the format of gemv_p13_kernel.h.
#include "gemv_p13_kernel.h"

CAKE_API int cake_swiglu_p13(int dt, const float* resid, const void* norm_w, float eps,
                             const void* pg, const void* pu, const int* hg, const int* hu,
                             const void* rg, const void* ru, int K, int I, void* act,
                             hipStream_t st) {
  if (p13_bad(dt, K, pg, hg) || p13_bad(dt, K, pu, hu)) return (int)hipErrorInvalidValue;
  return launch_swiglu<P13>(dt, resid, norm_w, eps, {(const uint8_t*)pg, hg, (const uint16_t*)rg},
                            {(const uint8_t*)pu, hu, (const uint16_t*)ru}, K, I, act, st);
}

CAKE_API int cake_gemv_x16_p13(int dt, const void* x, const void* planes, const int* hdr,
                               const void* raw, int K, int N, float* out, int accumulate,
                               hipStream_t st) {
  if (p13_bad(dt, K, planes, hdr)) return (int)hipErrorInvalidValue;
  return launch_x16<P13>(dt, x, {(const uint8_t*)planes, hdr, (const uint16_t*)raw}, K, N, out,
                         accumulate, st);
}
