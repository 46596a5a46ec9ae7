// MXFP4 weight-only decode projections: the tuning entry points and the QKV + RoPE one.
// Format: gemv_w4_kernel.h; SwiGLU: gemv_w4_mlp.hip; o_proj / down_proj:
// gemv_w4_x16.hip.  Arguments and semantics are those of cake_qkv_rope (gemv.hip) with
// packed 4-bit weights and one array of block-scale bytes per weight.
#include "gemv_w4_kernel.h"

CAKE_API int cake_gemv_w4_set_tuning(int kind, int U, int prefetch, int max_blocks) {
  return gemv_set_tuning<W4>(kind, U, prefetch, max_blocks);
}

CAKE_API int cake_gemv_w4_get_tuning(int kind, int* out3) { return gemv_get_tuning<W4>(kind, out3); }

// kv_fmt: the cache's format, as cake_qkv_rope_kvf (gemv.hip)
CAKE_API int cake_qkv_rope_w4_kvf(int dt, const float* resid, const void* norm_w, float eps,
                                  const void* wq, const void* wk, const void* wv, const void* eq,
                                  const void* ek, const void* ev, int K, int nh, int nkv, int hd,
                                  const float* inv_freq, const int* pos, float* q_out,
                                  void* kcache, void* vcache, int S, hipStream_t st, int kv_fmt) {
  return launch_qkv<W4>(dt, {resid, (const uint16_t*)norm_w, eps,
                             {(const uint8_t*)wq, (const uint8_t*)eq}, {(const uint8_t*)wk, (const uint8_t*)ek},
                             {(const uint8_t*)wv, (const uint8_t*)ev}, K, nh, nkv, hd, inv_freq, pos, q_out,
                             (uint16_t*)kcache, (uint16_t*)vcache, S, kv_fmt}, st);
}

CAKE_API int cake_qkv_rope_w4(int dt, const float* resid, const void* norm_w, float eps,
                              const void* wq, const void* wk, const void* wv, const void* eq,
                              const void* ek, const void* ev, int K, int nh, int nkv, int hd,
                              const float* inv_freq, const int* pos, float* q_out, void* kcache,
                              void* vcache, int S, hipStream_t st) {
  return cake_qkv_rope_w4_kvf(dt, resid, norm_w, eps, wq, wk, wv, eq, ek, ev, K, nh, nkv, hd,
                              inv_freq, pos, q_out, kcache, vcache, S, st, 0);
}
