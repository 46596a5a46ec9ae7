// P13 (lossless 13-bit bf16) lm_head entry points: the f32-output RMSNorm GEMV and the fused
// greedy tail, cake_gemv_norm_f32 / cake_head_select (gemv_head.hip) over the format of
// gemv_p13_kernel.h; the embedding table of the fused tail stays 16-bit.
#include "gemv_p13_kernel.h"

CAKE_API int cake_gemv_norm_f32_p13(int dt, const float* resid, const void* norm_w, float eps,
                                    const void* planes, const int* hdr, const void* raw, int K,
                                    int N, float* out, hipStream_t st) {
  if (p13_bad(dt, K, planes, hdr)) return (int)hipErrorInvalidValue;
  return launch_norm_f32<P13, false>(dt, resid, norm_w, eps,
                                     {(const uint8_t*)planes, hdr, (const uint16_t*)raw}, K, N,
                                     out, HeadSel{}, st);
}

CAKE_API int cake_head_select_p13(int dt, const float* resid, const void* norm_w, float eps,
                                  const void* planes, const int* hdr, const void* raw, int K,
                                  int N, float* out, int* hist, int* hist_len, int last_n,
                                  float penalty, unsigned long long* slot, unsigned int* ticket,
                                  int* tok, int* pos, int max_hist, const void* embed,
                                  float* emb_out, hipStream_t st) {
  if (p13_bad(dt, K, planes, hdr)) return (int)hipErrorInvalidValue;
  return launch_head_select<P13>(dt, resid, norm_w, eps,
                                 {(const uint8_t*)planes, hdr, (const uint16_t*)raw}, K, N, out,
                                 hist, hist_len, last_n, penalty, slot, ticket, tok, pos,
                                 max_hist, embed, emb_out, st);
}
