// Batch-1 decode projections: bandwidth-bound GEMV with fused prologues/epilogues.
//
// Replaces the reference's per-layer chain of candle ops for one decode token
// (SURVEY §2.4.1 K02 rms_norm, K03 Linear, K04 head-major copy, K05 rope,
// K06 kv cat, K14 residual add, K15 silu*mul, K17 logits cast), i.e.
//   cake-core/src/models/llama3/transformer.rs:51-73 (block forward),
//   cake-core/src/models/llama3/attention.rs:49-83 (q/k/v proj + rope),
//   cake-core/src/models/llama3/mlp.rs:15-18 (SwiGLU),
//   cake-core/src/models/llama3/llama.rs:119-137 (ln_f + lm_head -> f32).
//
// Design (MI355X-first):
//   * Weights stay in HF [out, in] row-major layout; every weight byte is read
//     exactly once per token with 16-byte non-temporal loads.
//   * One wave64 computes a PAIR of output rows so that the pair needs no
//     cross-wave communication in its epilogue:
//       - QKV:    rows (i, i + d/2) of one head -> RoPE rotation in registers,
//                 q written f32, k/v written straight into the preallocated
//                 KV cache slot [kvh][pos][d] (no cat, no transpose kernel).
//       - SwiGLU: gate row j and up row j -> act[j] = silu(g) * u.
//       - Resid:  rows (2p, 2p+1) -> residual stream += W x (in place, f32).
//       - F32:    rows (2p, 2p+1) -> f32 output (lm_head logits).
//   * RMSNorm is a block prologue: the f32 residual row is normalised into LDS
//     once per workgroup (4 waves), so no separate norm launch exists.
//   * The token position is read from device memory so the launches replay
//     unchanged inside a hipGraph.
#include "gemv_kernel.h"

namespace cake {
GemvTune g_tune[4][kNumKinds] = {
    // W16.  Measured in the decode graph (8B, tok/s):
    // profiles/r2_gemv_split_prologue_sweep*.jsonl — prefetching the first weight rows
    // behind the split x prologue is +10% (323 -> 357); the round-3 re-sweep
    // (profiles/r3_decode_gemv_tuning_ingraph.jsonl) moved QKV to U 2 / PF 4 (+0.3 %, every
    // round) and left the rest
    {{2, 4, 1024}, {2, 4, 512}, {4, 4, 1024}, {4, 4, 256}, {4, 4, 1024}},
    // W8: the whole 4096-byte row of an 8B projection in the prefetch registers; measured in
    // the 8B decode graph, one kind varied at a time
    // (profiles/fp8_decode_tuning_sweep.jsonl): SwiGLU at a 1024-block cap is -3..-5 %
    // ms/token against the 16-bit twin's 512 (rows are half as long, so a wave's fixed
    // prologue weighs twice as much per pair); every other variation stayed inside the 2 %
    // engine-to-engine spread of that sweep.  The fourth kind is the quantised lm_head,
    // started from the SwiGLU values
    {{2, 4, 1024}, {2, 4, 1024}, {4, 4, 1024}, {2, 4, 1024}},
    // W4: PF 4 runs as the deepest prefetch the row fills (W4::prefetch): the whole row of a
    // hidden-width projection at 8B (2 chunks per lane) and at 70B (4).  Measured in the 8B
    // decode graph, one kind varied at a time (profiles/mxfp4_decode_tuning_sweep.jsonl):
    // the prefetch is worth 4-8 % ms/token per kind, the SwiGLU cap of 1024 beats 512 and
    // 2048; every other variation stayed under twice the 1.2 % spread of the default (x16
    // at U = 1 was -1.4 to -2 %) and was not adopted.  Nothing was swept at 70B.  The fourth
    // kind is the quantised lm_head, started from the SwiGLU values.
    {{2, 4, 1024}, {2, 4, 1024}, {2, 4, 1024}, {2, 4, 1024}},
    // P13 (gemv_p13_kernel.h): a chunk is four W16 chunks, so U 1 / prefetch 1 are W16's
    // U 4 / prefetch 4; the grid caps are W16's but the lm_head's: at W16's 256 blocks (one
    // wave per SIMD) the packed head ran 185 us against the 16-bit head's 155, at 512 / 1024 /
    // 2048 blocks 133.5 / 148.7 / 136.8 (profiles/pack13_decode_tuning_sweep.jsonl)
    {{1, 1, 1024}, {1, 1, 512}, {1, 1, 1024}, {1, 1, 512}, {1, 1, 1024}}};
}  // namespace cake

CAKE_API int cake_gemv_set_tuning(int kind, int U, int prefetch, int max_blocks) {
  return gemv_set_tuning<W16>(kind, U, prefetch, max_blocks);
}

CAKE_API int cake_qkv_rope_kvf(int dt, const float* resid, const void* norm_w, float eps,
                               const void* wq, const void* wk, const void* wv, int K, int nh,
                               int nkv, int hd, const float* inv_freq, const int* pos,
                               float* q_out, void* kcache, void* vcache, int S,
                               hipStream_t st, int kv_fmt) {
  return launch_qkv<W16>(dt, {resid, (const uint16_t*)norm_w, eps, {(const uint16_t*)wq},
                              {(const uint16_t*)wk}, {(const uint16_t*)wv}, K, nh, nkv, hd,
                              inv_freq, pos, q_out, (uint16_t*)kcache, (uint16_t*)vcache, S,
                              kv_fmt}, st);
}

CAKE_API int cake_qkv_rope(int dt, const float* resid, const void* norm_w, float eps,
                           const void* wq, const void* wk, const void* wv, int K, int nh,
                           int nkv, int hd, const float* inv_freq, const int* pos,
                           float* q_out, void* kcache, void* vcache, int S,
                           hipStream_t st) {
  return cake_qkv_rope_kvf(dt, resid, norm_w, eps, wq, wk, wv, K, nh, nkv, hd, inv_freq, pos,
                           q_out, kcache, vcache, S, st, 0);
}
