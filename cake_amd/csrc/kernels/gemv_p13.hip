// P13 (lossless 13-bit bf16) decode projections: the tuning table and entry points of the
// format, and the QKV + RoPE kernel.  Format: gemv_p13_kernel.h; SwiGLU and the 16-bit-input
// GEMV: gemv_p13_mlp.hip; the lm_head: gemv_p13_head.hip.  Arguments and semantics are those
// of cake_qkv_rope_kvf (gemv.hip) with each weight given as its planes, row headers and raw
// rows (null when it has none).  bf16 only; K a multiple of 2048.
#include "gemv_p13_kernel.h"

CAKE_API int cake_gemv_p13_set_tuning(int kind, int U, int prefetch, int max_blocks) {
  return gemv_set_tuning<P13>(kind, U, prefetch, max_blocks);
}

CAKE_API int cake_gemv_p13_get_tuning(int kind, int* out3) { return gemv_get_tuning<P13>(kind, out3); }

CAKE_API int cake_qkv_rope_p13_kvf(int dt, const float* resid, const void* norm_w, float eps,
                                   const void* pq, const void* pk, const void* pv, const int* hq,
                                   const int* hk, const int* hv, const void* rq, const void* rk,
                                   const void* rv, int K, int nh, int nkv, int hd,
                                   const float* inv_freq, const int* pos, float* q_out,
                                   void* kcache, void* vcache, int S, hipStream_t st, int kv_fmt) {
  if (p13_bad(dt, K, pq, hq) || p13_bad(dt, K, pk, hk) || p13_bad(dt, K, pv, hv))
    return (int)hipErrorInvalidValue;
  return launch_qkv<P13>(dt, {resid, (const uint16_t*)norm_w, eps,
                              {(const uint8_t*)pq, hq, (const uint16_t*)rq},
                              {(const uint8_t*)pk, hk, (const uint16_t*)rk},
                              {(const uint8_t*)pv, hv, (const uint16_t*)rv}, K, nh, nkv, hd,
                              inv_freq, pos, q_out, (uint16_t*)kcache, (uint16_t*)vcache, S,
                              kv_fmt}, st);
}
