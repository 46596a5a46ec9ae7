// MXFP4 lm_head launchers: the f32-output RMSNorm GEMV over packed 4-bit rows with one
// e8m0 scale byte per 32 elements, and the fused greedy tail.  cake_gemv_norm_f32 /
// cake_head_select (gemv_head.hip) with `w4` + `e8` in place of the 16-bit weight; the
// embedding table of the fused tail stays 16-bit.  Kernels: gemv_w4_kernel.h.
#include "gemv_w4_kernel.h"

template <bool SEL>
static int launch_norm_f32_w4(int dt, const float* resid, const void* norm_w, float eps,
                              const void* w4, const void* e8, int K, int N, float* out,
                              const HeadSel& hs, hipStream_t st) {
  if (K < 32 || K % 32 || N < 1) return (int)hipErrorInvalidValue;
  const size_t lds = x32_lds_bytes4(K);
  const GemvTune t = g_tune_w4[kHeadW4];
  DISPATCH_DT(dt, DISPATCH_W4_TUNE(t, K, CAKE_NX_NORM(K, hipLaunchKernelGGL((gemv_norm_f32_w4_kernel<DT, U, PF, NX, SEL>),
                                                         dim3(grid_for((N + 1) / 2, t.MB)),
                                                         dim3(kGemvThreads), lds, st, resid,
                                                         (const uint16_t*)norm_w, eps,
                                                         (const uint8_t*)w4, (const uint8_t*)e8,
                                                         K, N, out, hs))));
  return (int)hipGetLastError();
}

CAKE_API int cake_gemv_norm_f32_w4(int dt, const float* resid, const void* norm_w, float eps,
                                   const void* w4, const void* e8, int K, int N, float* out,
                                   hipStream_t st) {
  return launch_norm_f32_w4<false>(dt, resid, norm_w, eps, w4, e8, K, N, out, HeadSel{}, st);
}

// slot (u64) and ticket (u32) must be zero before the first launch; the kernel re-arms
// them.  last_n <= 256.
CAKE_API int cake_head_select_w4(int dt, const float* resid, const void* norm_w, float eps,
                                 const void* w4, const void* e8, int K, int N, float* out,
                                 int* hist, int* hist_len, int last_n, float penalty,
                                 unsigned long long* slot, unsigned int* ticket, int* tok,
                                 int* pos, int max_hist, const void* embed, float* emb_out,
                                 hipStream_t st) {
  if (last_n < 0 || last_n > 256 || !(penalty > 0.f) || slot == nullptr || ticket == nullptr ||
      (embed != nullptr && emb_out == nullptr))
    return (int)hipErrorInvalidValue;
  const HeadSel hs{hist, hist_len, last_n, penalty, slot, ticket, tok, hist, hist_len, pos,
                   max_hist, (const uint16_t*)embed, emb_out, K};
  return launch_norm_f32_w4<true>(dt, resid, norm_w, eps, w4, e8, K, N, out, hs, st);
}
