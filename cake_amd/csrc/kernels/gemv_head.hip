// Decode GEMV entry points: the f32-output RMSNorm GEMV (lm_head) and the fused greedy
// tail (lm_head + repeat penalty + argmax + step finalize).  Kernels: gemv_kernel.h.
#include "gemv_kernel.h"

CAKE_API int cake_gemv_norm_f32(int dt, const float* resid, const void* norm_w, float eps,
                                const void* w, int K, int N, float* out, hipStream_t st) {
  return launch_norm_f32<W16, false>(dt, resid, norm_w, eps, {(const uint16_t*)w}, K, N, out,
                                     HeadSel{}, st);
}

CAKE_API int cake_head_select(int dt, const float* resid, const void* norm_w, float eps,
                              const void* w, int K, int N, float* out, int* hist, int* hist_len,
                              int last_n, float penalty, unsigned long long* slot,
                              unsigned int* ticket, int* tok, int* pos, int max_hist,
                              const void* embed, float* emb_out, hipStream_t st) {
  return launch_head_select<W16>(dt, resid, norm_w, eps, {(const uint16_t*)w}, K, N, out, hist,
                                 hist_len, last_n, penalty, slot, ticket, tok, pos, max_hist,
                                 embed, emb_out, st);
}
