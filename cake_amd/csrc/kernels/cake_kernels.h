// Public C ABI of libcake_kernels.so: every exported entry point of csrc/kernels,
// csrc/driver/blaslt.cpp and csrc/experimental, declared exactly once, plus the constants
// callers share with the kernels.  (cake_graph_decode and its structs: driver/graph_loop.h.)
//
// common.h includes this file, so every translation unit that defines an entry point sees
// its declaration and a definition whose types differ does not compile.  The engines and
// tools include it instead of writing prototypes; the ctypes table in ops/_lib.py mirrors it
// and tests/test_abi_cpu.py compares the two.  Adding an entry point: docs/ABI.md.
//
// Conventions: raw device pointers, the hipStream_t to launch on, hipError_t returned as int
// unless stated otherwise; dt is a cake::DType.  C++ only.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <hip/hip_runtime_api.h>

#define CAKE_API extern "C" __attribute__((visibility("default")))

namespace cake {

enum DType : int { kBF16 = 0, kF16 = 1, kF32 = 2 };

// epi of cake_gemm (cake_gemm_w8a8: kEpiStore, kEpiResid32, kEpiSwiglu only)
enum GemmEpi : int {
  kEpiStore = 0,   // C16 = acc (+ bias)
  kEpiResid32 = 1, // R32 += acc (+ bias)
  kEpiAdd16 = 2,   // C16 = acc (+ bias) + R16
  kEpiSwiglu = 3,  // C16[:, f] = silu(acc_gate) * acc_up
  kEpiGeglu = 4,   // C16[:, f] = acc_h * gelu_tanh(acc_gate)
  kEpiPartial = 5, // W32[split] = acc (split-K slab, virtual column order)
  kEpiStore32 = 6, // R32 = acc (+ bias)              (f32 output, e.g. conv time biases)
  kEpiSilu = 7,    // C16 = act(acc (+ bias)), act = GemmArgs::act: SiLU (time-embedding
                   // MLP), quick_gelu / erf-GELU (CLIP MLP)
  kEpiQuickGelu = 8,  // host ids only: cake_gemm runs 8 / 9 as the kEpiSilu kernel with
  kEpiGelu = 9,       // GemmArgs::act 1 / 2
};

// kv_fmt of the *_kvf writers (CakeEngineOpts.kv_fmt; oracle: ops/reference.py quant_kv_fp8)
// 0: 16-bit cache; 1: one OCP e4m3fn code per element, no scale; 2: the code's value kept in
// a 16-bit cache (exact in bf16 and f16: the test oracle of format 1).
enum KvFmt : int { kKv16 = 0, kKvFp8 = 1, kKvFp8Emu = 2 };

constexpr int kMaxSplit = 64;  // decode attention: splits per kv head (part: [nh][64][hd + 2])
constexpr int kHeadSelectMaxLastN = 256;  // cake_head_select*: repeat-penalty window bound
constexpr int kLpMaxK = 20;      // cake_logprob_topk: most alternatives per token
constexpr int kLpRecWords = 48;  // cake_logprob_topk: 32-bit words per record (192 bytes)
constexpr int kLcMaxBias = 300;     // cake_logit_controls: most logit_bias entries (OpenAI's limit)
constexpr int kLcParamWords = 608;  // cake_logit_controls: 32-bit words of the parameter block
constexpr int kLcStateWords = 68;   // cake_logit_controls: 32-bit words of the state block

}  // namespace cake

extern "C" {

// ---- kernels/allreduce.hip -------------------------------------------------------------
long long cake_ar_inbox_words(int world, int n);
int cake_ar_sum(const float* partial, float* out, int n, int accumulate, void* const* peers,
                const void* inbox, unsigned int* seq, int* err, int rank, int world,
                double timeout_s, hipStream_t st);
int cake_ar_max_key(unsigned long long* slot, void* const* peers, const void* inbox,
                    unsigned int* seq, int* err, int rank, int world, double timeout_s,
                    hipStream_t st);
int cake_ar_gather(const float* shard, int off, int n_local, float* full, int n,
                   void* const* peers, const void* inbox, unsigned int* seq, int* err, int rank,
                   int world, double timeout_s, hipStream_t st);

// ---- kernels/attention.hip -------------------------------------------------------------
int cake_attn_set_impl(int impl);
int cake_attn_set_stamps(void* p);
int cake_attn_set_split_cap(int cap);
int cake_attn_set_target_splits(int target);
int cake_attn_set_prefetch(int depth);
int cake_attn_set_single_max(int keys);
int cake_attn_debug_drop_partials(int on);
int cake_attn_splits(int Tk);
int cake_attn_max_split(int S);
int cake_attn_set_min_keys(int min_keys);
int cake_attn_decode(int dt, const float* q, const void* kc, const void* vc, const int* pos, int S,
                     int nh, int nkv, int hd, float scale, float* part, unsigned int* tickets,
                     void* out, hipStream_t st);
// the decode attention over an FP8 e4m3 KV cache (one code per element)
int cake_attn_decode_kv8(int dt, const float* q, const void* kc8, const void* vc8, const int* pos,
                         int S, int nh, int nkv, int hd, float scale, float* part,
                         unsigned int* tickets, void* out, hipStream_t st);
int cake_attn_set_head_prefetch(int pfd);
int cake_attn_set_heads(int max_keys, int waves);
int cake_attn_heads_max();
int cake_attn_decode_heads(int dt, const float* q, const void* kc, const void* vc, const int* pos,
                           int S, int nh, int nkv, int hd, float scale, void* out, hipStream_t st);

// ---- kernels/attn512.hip ---------------------------------------------------------------
int cake_attn512(int dt, const void* q, const void* k, const void* v, void* o, int B, int N, int M,
                 long long sq, long long sk, long long sv, long long so, long long bq,
                 long long bk, long long bv, long long bo, float scale, const void* zeros,
                 hipStream_t st);

// ---- kernels/conv2d.hip ----------------------------------------------------------------
int cake_conv1x1_small(int dt, const void* x, const void* w, const void* bias, void* out, int N,
                       int HW, int IC, int OC, int layout, hipStream_t st);
long long cake_conv2d_workspace(int P, int OC, int splits);
int cake_conv2d_nhwc2(int dt, const void* x, const void* w, const void* bias, const float* bias2,
                      const void* resid, void* out, float* ws, const void* zeros, int N, int H,
                      int W, int IC, int OC, int KH, int KW, int stride, int pad, int up, int cfg,
                      int splits, int th, int tw, int bias2_ld, int layout, hipStream_t st);
int cake_conv2d_nhwc(int dt, const void* x, const void* w, const void* bias, const float* bias2,
                     const void* resid, void* out, float* ws, const void* zeros, int N, int H,
                     int W, int IC, int OC, int KH, int KW, int stride, int pad, int up, int cfg,
                     int splits, int th, int tw, int bias2_ld, hipStream_t st);

// ---- kernels/elementwise.hip -----------------------------------------------------------
int cake_sum_slices(float* out, const float* src, int W, long long stride, long long n,
                    int accumulate, hipStream_t st);
int cake_stream_read(const void* p, size_t bytes, int blocks, unsigned int* sink, hipStream_t st);
int cake_cast16(int src_kind, int dt, const void* src, void* dst, size_t n, hipStream_t st);
int cake_fill_normal(int dt, void* dst, size_t n, float mean, float std, unsigned long long key,
                     hipStream_t st);
int cake_embed(int dt, const void* table, const int* tok, int T, int H, float* out,
               hipStream_t st);
void cake_rmsnorm_set_reg(int on);
int cake_rmsnorm(int dt, const float* x, const void* w, float eps, int T, int H, void* out,
                 hipStream_t st);
int cake_rope_kv(int dt, void* q, const void* k, const void* v, int ldq, int ld, int T, int nh,
                 int nkv, int hd, const float* inv_freq, int pos0, int S, void* kc, void* vc,
                 hipStream_t st);
// The KV writers with the cache's format as their last argument (cake::KvFmt; kKv16 = the
// 16-bit entry points cake_qkv_rope* / cake_rope_kv), and the prefill read of an FP8 cache
int cake_rope_kv_kvf(int dt, void* q, const void* k, const void* v, int ldq, int ld, int T, int nh,
                     int nkv, int hd, const float* inv_freq, int pos0, int S, void* kc, void* vc,
                     hipStream_t st, int kv_fmt);
int cake_dequant_kv_fp8(int dt, const void* k8, const void* v8, int nkv, int S, int hd, int Tk,
                        void* k16, void* v16, hipStream_t st);
int cake_silu_mul(int dt, const void* g, const void* u, size_t n, void* out, hipStream_t st);
int cake_silu_mul_rows(int dt, const void* gu, size_t T, int I, void* out, hipStream_t st);
int cake_add_resid(int dt, float* resid, const void* y, size_t n, hipStream_t st);
int cake_wave_reduce_probe(const float* x, float* out, hipStream_t st);

// ---- kernels/flash_attn.hip ------------------------------------------------------------
void cake_flash_set_impl(int v);
void cake_flash_set_nw(int nw);
void cake_flash_set_pair_min(long long n);
void cake_flash_set_ksplit(int k);
int cake_flash_attn_ws(int dt, const void* q, const void* k, const void* v, void* o, int B, int H,
                       int Hkv, int N, int M, int D, const long long* strides, float scale,
                       int causal, int pos0, void* ws, long long ws_bytes, hipStream_t st);
int cake_flash_attn(int dt, const void* q, const void* k, const void* v, void* o, int B, int H,
                    int Hkv, int N, int M, int D, const long long* strides, float scale,
                    int causal, int pos0, hipStream_t st);

// ---- kernels/gemm.hip ------------------------------------------------------------------
int cake_gemm_tile(int cfg, int* bm, int* bn);
// f32 elements of workspace a cake_gemm call with these arguments needs (0: unsplit)
long long cake_gemm_ws_floats(int cfg, int splits, int M, int N, int K, int gated);
// epi: a cake::GemmEpi
int cake_gemm(int dt, int epi, int cfg, int splits, const void* a, long long lda, const void* b,
              long long ldb, void* c, long long ldc, const void* bias, void* resid, long long ldr,
              float* ws, const void* zeros, int M, int N, int K, hipStream_t st);

// ---- kernels/gemm_w8a8.hip -------------------------------------------------------------
int cake_gemm_w8a8_num_cfgs();
int cake_gemm_w8a8_plan(int M, int Nv, int K);
// FP8 x FP8 MFMA GEMM of the quantised prefill: e4m3 activation codes with one f32 scale per
// token against the resident projection codes; cfg < 0 = its planner's tile
int cake_gemm_w8a8(int dt, int epi, int cfg, const void* a8, long long lda, const float* sa,
                   const void* w8, long long ldb, const float* sw, void* c, long long ldc,
                   float* r32, long long ldr, int M, int N, int K, hipStream_t st);

// ---- kernels/gemv.hip ------------------------------------------------------------------
int cake_gemv_set_tuning(int kind, int U, int prefetch, int max_blocks);
int cake_qkv_rope_kvf(int dt, const float* resid, const void* norm_w, float eps, const void* wq,
                      const void* wk, const void* wv, int K, int nh, int nkv, int hd,
                      const float* inv_freq, const int* pos, float* q_out, void* kcache,
                      void* vcache, int S, hipStream_t st, int kv_fmt);
int cake_qkv_rope(int dt, const float* resid, const void* norm_w, float eps, const void* wq,
                  const void* wk, const void* wv, int K, int nh, int nkv, int hd,
                  const float* inv_freq, const int* pos, float* q_out, void* kcache, void* vcache,
                  int S, hipStream_t st);

// ---- kernels/gemv_head.hip -------------------------------------------------------------
int cake_gemv_norm_f32(int dt, const float* resid, const void* norm_w, float eps, const void* w,
                       int K, int N, float* out, hipStream_t st);
// last_n <= cake::kHeadSelectMaxLastN (also the _w8 / _w4 forms)
int cake_head_select(int dt, const float* resid, const void* norm_w, float eps, const void* w,
                     int K, int N, float* out, int* hist, int* hist_len, int last_n, float penalty,
                     unsigned long long* slot, unsigned int* ticket, int* tok, int* pos,
                     int max_hist, const void* embed, float* emb_out, hipStream_t st);

// ---- kernels/gemv_mlp.hip --------------------------------------------------------------
int cake_swiglu(int dt, const float* resid, const void* norm_w, float eps, const void* wg,
                const void* wu, int K, int I, void* act, hipStream_t st);
int cake_gemv_x16(int dt, const void* x, const void* w, int K, int N, float* out, int accumulate,
                  hipStream_t st);

// ---- kernels/gemv_p13.hip: lossless 13-bit bf16 projections (with pack13.hip) ----------
// every P13 weight is (planes, row headers, raw rows or null); bf16 only, K % 2048 == 0
int cake_gemv_p13_set_tuning(int kind, int U, int prefetch, int max_blocks);
int cake_gemv_p13_get_tuning(int kind, int* out3);
int cake_qkv_rope_p13_kvf(int dt, const float* resid, const void* norm_w, float eps,
                          const void* pq, const void* pk, const void* pv, const int* hq,
                          const int* hk, const int* hv, const void* rq, const void* rk,
                          const void* rv, int K, int nh, int nkv, int hd, const float* inv_freq,
                          const int* pos, float* q_out, void* kcache, void* vcache, int S,
                          hipStream_t st, int kv_fmt);

// ---- kernels/gemv_p13_head.hip: the packed lm_head -------------------------------------
int cake_gemv_norm_f32_p13(int dt, const float* resid, const void* norm_w, float eps,
                           const void* planes, const int* hdr, const void* raw, int K, int N,
                           float* out, hipStream_t st);
int cake_head_select_p13(int dt, const float* resid, const void* norm_w, float eps,
                         const void* planes, const int* hdr, const void* raw, int K, int N,
                         float* out, int* hist, int* hist_len, int last_n, float penalty,
                         unsigned long long* slot, unsigned int* ticket, int* tok, int* pos,
                         int max_hist, const void* embed, float* emb_out, hipStream_t st);

// ---- kernels/gemv_p13_mlp.hip ----------------------------------------------------------
int cake_swiglu_p13(int dt, const float* resid, const void* norm_w, float eps, const void* pg,
                    const void* pu, const int* hg, const int* hu, const void* rg, const void* ru,
                    int K, int I, void* act, hipStream_t st);
int cake_gemv_x16_p13(int dt, const void* x, const void* planes, const int* hdr, const void* raw,
                      int K, int N, float* out, int accumulate, hipStream_t st);

// ---- kernels/gemv_rows.hip: the projections of a lock-step batched decode step ---------
// epi: kEpiStore32, kEpiResid32 or kEpiSwiglu; tiles 1 / 2 / 4 (swiglu 1 / 2), unroll 2 / 4
int cake_gemv_rows_set_tuning(int epi, int tiles, int unroll, int max_blocks);
int cake_gemv_rows_get_tuning(int epi, int* out3);
// x16 [M, K] (dt) times the 16-bit rows w [N, K], 1 <= M <= 16, K % 32 == 0, ldx and ldw
// multiples of 8.  store32: out f32 [M, N] = sum; resid32: resid32 f32 [M, N] += sum;
// swiglu: out 16-bit [M, N] = silu(w[n] . x) * (w[N + n] . x), w the packed [2N, K].
int cake_gemv_rows(int dt, int epi, const void* x16, long long ldx, const void* w, long long ldw,
                   void* out, long long ldo, float* resid32, long long ldr, int M, int N, int K,
                   hipStream_t st);
// RMSNorm of x f32 [M, H], M <= 8, as two 16-bit terms, out16 [2M, H]: row m = cake_rmsnorm's
// row, row M + m = the rounded remainder of the f32 value (the batched lm_head's operand)
int cake_rmsnorm_split_rows(int dt, const float* x, const void* w, float eps, int M, int H,
                            void* out16, hipStream_t st);
// qkv32 f32 [M, (nh + 2 nkv) hd] -> q_out f32 [M, nh hd] roped, k roped and v into row pos[m]
// of the 16-bit caches at kbase[m] / vbase[m] + layer_off elements ([nkv][S][hd]); pos, kbase
// and vbase are device arrays of M entries; a row with pos[m] outside [0, S) writes nothing
int cake_rope_kv_rows(int dt, const float* qkv32, long long ldq, int M, const int* pos,
                      const float* inv_freq, int nh, int nkv, int hd, int S, float* q_out,
                      void* const* kbase, void* const* vbase, long long layer_off,
                      hipStream_t st);

// ---- kernels/gemv_w4.hip: MXFP4 weight-only projections (with quant_mxfp4.hip) ---------
int cake_gemv_w4_set_tuning(int kind, int U, int prefetch, int max_blocks);
int cake_gemv_w4_get_tuning(int kind, int* out3);
int cake_qkv_rope_w4_kvf(int dt, const float* resid, const void* norm_w, float eps, const void* wq,
                         const void* wk, const void* wv, const void* eq, const void* ek,
                         const void* ev, int K, int nh, int nkv, int hd, const float* inv_freq,
                         const int* pos, float* q_out, void* kcache, void* vcache, int S,
                         hipStream_t st, int kv_fmt);
int cake_qkv_rope_w4(int dt, const float* resid, const void* norm_w, float eps, const void* wq,
                     const void* wk, const void* wv, const void* eq, const void* ek,
                     const void* ev, int K, int nh, int nkv, int hd, const float* inv_freq,
                     const int* pos, float* q_out, void* kcache, void* vcache, int S,
                     hipStream_t st);

// ---- kernels/gemv_w4_head.hip: quantised lm_head ---------------------------------------
int cake_gemv_norm_f32_w4(int dt, const float* resid, const void* norm_w, float eps,
                          const void* w4, const void* e8, int K, int N, float* out,
                          hipStream_t st);
int cake_head_select_w4(int dt, const float* resid, const void* norm_w, float eps, const void* w4,
                        const void* e8, int K, int N, float* out, int* hist, int* hist_len,
                        int last_n, float penalty, unsigned long long* slot, unsigned int* ticket,
                        int* tok, int* pos, int max_hist, const void* embed, float* emb_out,
                        hipStream_t st);

// ---- kernels/gemv_w4_mlp.hip -----------------------------------------------------------
int cake_swiglu_w4(int dt, const float* resid, const void* norm_w, float eps, const void* wg,
                   const void* wu, const void* eg, const void* eu, int K, int I, void* act,
                   hipStream_t st);

// ---- kernels/gemv_w4_x16.hip -----------------------------------------------------------
int cake_gemv_x16_w4(int dt, const void* x, const void* w, const void* e8, int K, int N,
                     float* out, int accumulate, hipStream_t st);

// ---- kernels/gemv_w8.hip: FP8 e4m3fn weight-only projections (with quant_fp8.hip) ------
int cake_gemv_w8_set_tuning(int kind, int U, int prefetch, int max_blocks);
int cake_gemv_w8_get_tuning(int kind, int* out3);
int cake_qkv_rope_w8_kvf(int dt, const float* resid, const void* norm_w, float eps, const void* wq,
                         const void* wk, const void* wv, const float* sq, const float* sk,
                         const float* sv, int K, int nh, int nkv, int hd, const float* inv_freq,
                         const int* pos, float* q_out, void* kcache, void* vcache, int S,
                         hipStream_t st, int kv_fmt);
int cake_qkv_rope_w8(int dt, const float* resid, const void* norm_w, float eps, const void* wq,
                     const void* wk, const void* wv, const float* sq, const float* sk,
                     const float* sv, int K, int nh, int nkv, int hd, const float* inv_freq,
                     const int* pos, float* q_out, void* kcache, void* vcache, int S,
                     hipStream_t st);

// ---- kernels/gemv_w8_head.hip: quantised lm_head ---------------------------------------
int cake_gemv_norm_f32_w8(int dt, const float* resid, const void* norm_w, float eps,
                          const void* w8, const float* scale, int K, int N, float* out,
                          hipStream_t st);
int cake_head_select_w8(int dt, const float* resid, const void* norm_w, float eps, const void* w8,
                        const float* scale, int K, int N, float* out, int* hist, int* hist_len,
                        int last_n, float penalty, unsigned long long* slot, unsigned int* ticket,
                        int* tok, int* pos, int max_hist, const void* embed, float* emb_out,
                        hipStream_t st);

// ---- kernels/gemv_w8_mlp.hip -----------------------------------------------------------
int cake_swiglu_w8(int dt, const float* resid, const void* norm_w, float eps, const void* wg,
                   const void* wu, const float* sg, const float* su, int K, int I, void* act,
                   hipStream_t st);

// ---- kernels/gemv_w8_x16.hip -----------------------------------------------------------
int cake_gemv_x16_w8(int dt, const void* x, const void* w, const float* scale, int K, int N,
                     float* out, int accumulate, hipStream_t st);

// ---- kernels/hop.hip -------------------------------------------------------------------
int cake_hop_alloc(size_t bytes, void** ptr);
int cake_hop_free(void* ptr);
int cake_ipc_handle(void* ptr, void* out64);
int cake_ipc_handle_size();
int cake_ipc_open(const void* in64, void** ptr);
int cake_ipc_close(void* ptr);
int cake_hop_words(int H, int nhdr, int bf16);
int cake_hop_send(const float* src, int H, int nhdr, int bf16, void* dst_inbox, unsigned int* seq,
                  hipStream_t st);
int cake_hop_recv(const void* inbox, int H, int nhdr, int bf16, float* dst, unsigned int* seq,
                  int* err, double timeout_s, hipStream_t st);
int cake_bulk_send(const void* const* srcs, const unsigned long long* bytes,
                   const unsigned long long* offs, int nseg, void* dst_rx,
                   unsigned long long rx_bytes, unsigned int* seq, unsigned int* count,
                   hipStream_t st);
int cake_bulk_recv(const void* rx, unsigned long long bytes, void* dst, unsigned int* seq,
                   int* err, double timeout_s, hipStream_t st);

// ---- kernels/logit_controls.hip: count penalties, logit_bias and the min_p cut ---------
// params: cake::kLcParamWords words, state: cake::kLcStateWords words, cnt: V words
int cake_logit_controls(float* logits, int V, const int32_t* hist, const int32_t* hist_len,
                        unsigned int* cnt, const void* params, unsigned int* state,
                        int max_blocks, hipStream_t st);
int cake_logit_controls_merge_thr(unsigned int* thr, const unsigned int* cut, hipStream_t st);

// ---- kernels/logprob.hip: log-probs of a generated token -------------------------------
long long cake_logprob_ws_bytes(int V);
// one record of cake::kLpRecWords words at rec[*hist_len - 1]; K <= cake::kLpMaxK
int cake_logprob_topk(const float* logits, int V, const int32_t* tok, const int32_t* hist_len,
                      int K, void* rec, int max_rec, void* ws, unsigned int* ticket,
                      int max_blocks, hipStream_t st);

// ---- kernels/pack13.hip: bf16 rows <-> their lossless 13-bit form ----------------------
// bytes of planes | headers | nraw raw rows of a packed [N, K]; -1: K is not whole tiles
long long cake_pack13_bytes(int N, int K, int nraw);
// kind: a cake::PackKind (the row pairing of the reading kernel).  Returns the raw-row count
// or a negated hipError_t; planes, hdr and raw all null: the count only.  Synchronous.
int cake_pack13_rows(int kind, const void* rows16, int N, int K, int hd, void* planes, int* hdr,
                     void* raw, int raw_cap, hipStream_t st);
int cake_unpack13_rows(const void* planes, const int* hdr, const void* raw, int N, int K,
                       void* out16, hipStream_t st);

// ---- kernels/quant_fp8.hip -------------------------------------------------------------
int cake_quant_rows_fp8(int dt, const void* w16, int N, int K, void* w8, float* scale,
                        hipStream_t st);
int cake_dequant_rows_fp8(int dt, const void* w8, const float* scale, int N, int K, void* out16,
                          hipStream_t st);

// ---- kernels/quant_mxfp4.hip -----------------------------------------------------------
int cake_quant_rows_mxfp4(int dt, const void* w16, int N, int K, void* w4, void* e8,
                          hipStream_t st);
int cake_dequant_rows_mxfp4(int dt, const void* w4, const void* e8, int N, int K, void* out16,
                            hipStream_t st);

// ---- kernels/sampling.hip --------------------------------------------------------------
int cake_sample_threshold(const float* logits, int V, float temperature, int top_k, float top_p,
                          unsigned int* thr, hipStream_t st);
int cake_select_dev(const float* logits, int V, const void* params, const int* step,
                    unsigned int* thr, unsigned long long* slot, hipStream_t st);
int cake_gumbel_argmax(const float* logits, int V, float temperature, unsigned long long seed,
                       const int* step, const unsigned int* thr, unsigned long long* slot,
                       hipStream_t st);
int cake_repeat_penalty(float* logits, const int* hist, const int* hist_len, int last_n,
                        float penalty, hipStream_t st);
int cake_argmax(const float* logits, int V, unsigned long long* slot, hipStream_t st);
int cake_select_shard(float* logits, int V, int off, const int* hist, const int* hist_len,
                      int last_n, float penalty, float temperature, unsigned long long seed,
                      unsigned long long* slot, hipStream_t st);
int cake_finalize_token(unsigned long long* slot, int* tok, int* hist, int* hist_len, int* pos,
                        int max_hist, hipStream_t st);
int cake_push_token(const int* src, int* tok, int* hist, int* hist_len, int* pos, int max_hist,
                    hipStream_t st);

// ---- kernels/score.hip: sequence scoring -----------------------------------------------
// streaming log-sum-exp / target gather / argmax over one vocabulary chunk of f32 logits,
// per-row state carried from chunk to chunk
int cake_lse_rows(const float* logits, long long ld, int T, int Vc, int v0, int first,
                  const int32_t* target, float* run_max, double* run_sum, float* tgt,
                  unsigned long long* key, hipStream_t st);
int cake_lse_finish(const float* run_max, const double* run_sum, const unsigned long long* key,
                    int T, float* lse, int32_t* top, float* topv, hipStream_t st);

// ---- kernels/sd_norm.hip ---------------------------------------------------------------
int cake_groupnorm(int dt, const void* x, const void* gamma, const void* beta, int B, int C,
                   long long HW, int G, float eps, int silu_act, float* part, void* y,
                   hipStream_t st);
int cake_layernorm(int dt, const void* x, const void* gamma, const void* beta, long long rows,
                   int C, float eps, void* y, hipStream_t st);
int cake_geglu(int dt, const void* h, long long rows, int F, void* out, hipStream_t st);
int cake_groupnorm_nhwc_splits(int HW);
int cake_groupnorm_nhwc2(int dt, const void* x, const void* x2, int Cx, void* cat,
                         const void* gamma, const void* beta, int N, int HW, int C, int G,
                         float eps, int silu_act, double* part, unsigned int* tickets,
                         float* stats, void* y, hipStream_t st);
int cake_groupnorm_nhwc(int dt, const void* x, const void* gamma, const void* beta, int N, int HW,
                        int C, int G, float eps, int silu_act, double* part, unsigned int* tickets,
                        float* stats, void* y, hipStream_t st);

// ---- kernels/sd_small.hip --------------------------------------------------------------
int cake_timestep_embed(int dt, const float* t_table, const int* step, int B, int dim, int flip,
                        float shift, int out16, void* out, hipStream_t st);
int cake_sched_step(int dt, float* x, const void* pred, long long n, int cfg, float guidance,
                    const void* coef, const int* step, const void* seed, void* next_in,
                    hipStream_t st);
int cake_step_advance(int* step, hipStream_t st);
int cake_scale_copy(int dt, const float* x, long long n, float scale, int dup, void* out,
                    hipStream_t st);
int cake_to_rgb8(int dt, const void* img, int B, int H, int W, int nhwc, void* out,
                 hipStream_t st);
int cake_clip_embed(int dt, const void* tok, const void* pos, const int* ids, int rows, int T,
                    int D, int V, void* out, hipStream_t st);
int cake_widen16(int dt, const void* x, long long n, float* y, hipStream_t st);

// ---- driver/blaslt.cpp -----------------------------------------------------------------
// 0 on success, else a hipblasStatus_t (+1000 so it cannot read as a hipError_t 0..999)
int cake_blaslt_gemm(int dt, int out, const void* a, long long lda, const void* w, long long ldw,
                     void* c, long long ldc, int M, int N, int K, void* ws, size_t ws_bytes,
                     hipStream_t st);

// ==== experimental ======================================================================
// csrc/experimental: these exist only in a library built with CAKE_BUILD_EXPERIMENTAL=1.
// Callers look them up at run time (dlsym / ops/_lib.py _OPTIONAL) and never link to them.

// ---- experimental/attn_oproj.hip -------------------------------------------------------
int cake_attn_oproj_supported(int nh, int nkv, int hd, int H);
long long cake_attn_oproj_ws_floats(int nkv, int H);
long long cake_attn_oproj_ticket_words(int nkv, int H);
int cake_attn_oproj(int dt, const float* q, const void* kc, const void* vc, const int* pos, int S,
                    int nh, int nkv, int hd, float scale, const void* wo, int ldw, int H,
                    float* out, int accumulate, float* ws, unsigned int* tickets,
                    unsigned int* err, hipStream_t st);

// ---- experimental/decode_mk.hip --------------------------------------------------------
long long cake_mk_gstride(int H, int I, int nh, int nkv, int hd);
int cake_mk_grid();
int cake_mk_set_stamps(void* p);
int cake_mk_set_tuning(int thin, int ring, int fly, int o_all);
int cake_mk_supported(int H, int I, int nh, int nkv, int hd);
int cake_mk_decode(int dt, const void* layers, int L, int H, int I, int nh, int nkv, int hd, int S,
                   float eps, float scale, const float* inv_freq, const int* pos, float* resid,
                   void* gran, unsigned int* ctl, double timeout_s, hipStream_t st);

}  // extern "C"
