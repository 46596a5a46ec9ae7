// FP8 (e4m3fn) weight-only decode projections: the tuning table and the QKV + RoPE
// launcher.  Kernels and format: gemv_w8_kernel.h; SwiGLU: gemv_w8_mlp.hip; o_proj /
// down_proj: gemv_w8_x16.hip.  Arguments and semantics are those of cake_qkv_rope
// (gemv.hip) with byte weights and one f32 row-scale vector per weight.
#include "gemv_w8_kernel.h"

namespace cake {
// the whole 4096-byte row of an 8B projection in the prefetch registers; measured in the
// 8B decode graph, one kind varied at a time (profiles/fp8_decode_tuning_sweep.jsonl):
// SwiGLU at a 1024-block cap is -3..-5 % ms/token against the 16-bit twin's 512 (rows
// are half as long, so a wave's fixed prologue weighs twice as much per pair); every
// other variation stayed inside the 2 % engine-to-engine spread of that sweep.  The fourth
// kind is the quantised lm_head (gemv_w8_head.hip), started from the SwiGLU values
GemvTune g_tune_w8[kNumW8Kinds] = {{2, 4, 1024}, {2, 4, 1024}, {4, 4, 1024}, {2, 4, 1024}};
}  // namespace cake

CAKE_API int cake_gemv_w8_set_tuning(int kind, int U, int prefetch, int max_blocks) {
  if (kind < 0 || kind >= kNumW8Kinds || (U != 1 && U != 2 && U != 4) || max_blocks < 1 ||
      (prefetch != 0 && prefetch != 2 && prefetch != 4))
    return (int)hipErrorInvalidValue;
  g_tune_w8[kind] = GemvTune{U, prefetch, max_blocks};
  return 0;
}

CAKE_API int cake_gemv_w8_get_tuning(int kind, int* out3) {
  if (kind < 0 || kind >= kNumW8Kinds || !out3) return (int)hipErrorInvalidValue;
  out3[0] = g_tune_w8[kind].U;
  out3[1] = g_tune_w8[kind].PF;
  out3[2] = g_tune_w8[kind].MB;
  return 0;
}

// kv_fmt: the cache's format, as cake_qkv_rope_kvf (gemv.hip)
CAKE_API int cake_qkv_rope_w8_kvf(int dt, const float* resid, const void* norm_w, float eps,
                                  const void* wq, const void* wk, const void* wv, const float* sq,
                                  const float* sk, const float* sv, int K, int nh, int nkv, int hd,
                                  const float* inv_freq, const int* pos, float* q_out,
                                  void* kcache, void* vcache, int S, hipStream_t st, int kv_fmt) {
  if (K < 16 || K % 16 || hd % 2 || nh < 1 || nkv < 1 || kv_fmt < 0 || kv_fmt > 2)
    return (int)hipErrorInvalidValue;
  QkvW8Args a{resid, (const uint16_t*)norm_w, eps, (const uint8_t*)wq, (const uint8_t*)wk,
              (const uint8_t*)wv, sq, sk, sv, K, nh, nkv, hd, inv_freq, pos, q_out,
              (uint16_t*)kcache, (uint16_t*)vcache, S, kv_fmt};
  const int npairs = (nh + 2 * nkv) * (hd / 2);
  const size_t lds = x32_lds_bytes(K);
  const GemvTune t = g_tune_w8[kQkvW8];
  DISPATCH_DT(dt, DISPATCH_W8_TUNE(t, K, CAKE_NX_NORM(K, hipLaunchKernelGGL((qkv_rope_w8_kernel<DT, U, PF, NX>),
                                                         dim3(grid_for(npairs, t.MB)),
                                                         dim3(kGemvThreads), lds, st, a))));
  return (int)hipGetLastError();
}

CAKE_API int cake_qkv_rope_w8(int dt, const float* resid, const void* norm_w, float eps,
                              const void* wq, const void* wk, const void* wv, const float* sq,
                              const float* sk, const float* sv, int K, int nh, int nkv, int hd,
                              const float* inv_freq, const int* pos, float* q_out, void* kcache,
                              void* vcache, int S, hipStream_t st) {
  return cake_qkv_rope_w8_kvf(dt, resid, norm_w, eps, wq, wk, wv, sq, sk, sv, K, nh, nkv, hd,
                              inv_freq, pos, q_out, kcache, vcache, S, st, 0);
}
