// MXFP4 weight-only decode projections: the tuning table and the QKV + RoPE launcher.
// Kernels and format: gemv_w4_kernel.h; SwiGLU: gemv_w4_mlp.hip; o_proj / down_proj:
// gemv_w4_x16.hip.  Arguments and semantics are those of cake_qkv_rope (gemv.hip) with
// packed 4-bit weights and one array of block-scale bytes per weight.
#include "gemv_w4_kernel.h"

namespace cake {
// PF 4 runs as the deepest prefetch the row fills (DISPATCH_W4_TUNE): the whole row of a
// hidden-width projection at 8B (2 chunks per lane) and at 70B (4).  Measured in the 8B
// decode graph, one kind varied at a time (profiles/mxfp4_decode_tuning_sweep.jsonl): the
// prefetch is worth 4-8 % ms/token per kind, the SwiGLU cap of 1024 beats 512 and 2048;
// every other variation stayed under twice the 1.2 % spread of the default (x16 at U = 1
// was -1.4 to -2 %) and was not adopted.  Nothing was swept at 70B.  The fourth kind is the
// quantised lm_head (gemv_w4_head.hip), started from the SwiGLU values.
GemvTune g_tune_w4[kNumW4Kinds] = {{2, 4, 1024}, {2, 4, 1024}, {2, 4, 1024}, {2, 4, 1024}};
}  // namespace cake

CAKE_API int cake_gemv_w4_set_tuning(int kind, int U, int prefetch, int max_blocks) {
  if (kind < 0 || kind >= kNumW4Kinds || (U != 1 && U != 2 && U != 4) || max_blocks < 1 ||
      (prefetch != 0 && prefetch != 2 && prefetch != 4))
    return (int)hipErrorInvalidValue;
  g_tune_w4[kind] = GemvTune{U, prefetch, max_blocks};
  return 0;
}

CAKE_API int cake_gemv_w4_get_tuning(int kind, int* out3) {
  if (kind < 0 || kind >= kNumW4Kinds || !out3) return (int)hipErrorInvalidValue;
  out3[0] = g_tune_w4[kind].U;
  out3[1] = g_tune_w4[kind].PF;
  out3[2] = g_tune_w4[kind].MB;
  return 0;
}

// kv_fmt: the cache's format, as cake_qkv_rope_kvf (gemv.hip)
CAKE_API int cake_qkv_rope_w4_kvf(int dt, const float* resid, const void* norm_w, float eps,
                                  const void* wq, const void* wk, const void* wv, const void* eq,
                                  const void* ek, const void* ev, int K, int nh, int nkv, int hd,
                                  const float* inv_freq, const int* pos, float* q_out,
                                  void* kcache, void* vcache, int S, hipStream_t st, int kv_fmt) {
  if (K < 32 || K % 32 || hd % 2 || nh < 1 || nkv < 1 || kv_fmt < 0 || kv_fmt > 2)
    return (int)hipErrorInvalidValue;
  QkvW4Args a{resid, (const uint16_t*)norm_w, eps, (const uint8_t*)wq, (const uint8_t*)wk,
              (const uint8_t*)wv, (const uint8_t*)eq, (const uint8_t*)ek, (const uint8_t*)ev,
              K, nh, nkv, hd, inv_freq, pos, q_out, (uint16_t*)kcache, (uint16_t*)vcache, S,
              kv_fmt};
  const int npairs = (nh + 2 * nkv) * (hd / 2);
  const size_t lds = x32_lds_bytes4(K);
  const GemvTune t = g_tune_w4[kQkvW4];
  DISPATCH_DT(dt, DISPATCH_W4_TUNE(t, K, CAKE_NX_NORM(K, hipLaunchKernelGGL((qkv_rope_w4_kernel<DT, U, PF, NX>),
                                                         dim3(grid_for(npairs, t.MB)),
                                                         dim3(kGemvThreads), lds, st, a))));
  return (int)hipGetLastError();
}

CAKE_API int cake_qkv_rope_w4(int dt, const float* resid, const void* norm_w, float eps,
                              const void* wq, const void* wk, const void* wv, const void* eq,
                              const void* ek, const void* ev, int K, int nh, int nkv, int hd,
                              const float* inv_freq, const int* pos, float* q_out, void* kcache,
                              void* vcache, int S, hipStream_t st) {
  return cake_qkv_rope_w4_kvf(dt, resid, norm_w, eps, wq, wk, wv, eq, ek, ev, K, nh, nkv, hd,
                              inv_freq, pos, q_out, kcache, vcache, S, st, 0);
}
