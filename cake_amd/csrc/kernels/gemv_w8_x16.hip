// FP8 (e4m3fn) weight-only decode entry point: the 16-bit-input GEMV (o_proj / down_proj,
// optional residual accumulate), cake_gemv_x16 (gemv_mlp.hip) over the format of
// gemv_w8_kernel.h.
#include "gemv_w8_kernel.h"

CAKE_API int cake_gemv_x16_w8(int dt, const void* x, const void* w, const float* scale, int K,
                              int N, float* out, int accumulate, hipStream_t st) {
  return launch_x16<W8>(dt, x, {(const uint8_t*)w, scale}, K, N, out, accumulate, st);
}
