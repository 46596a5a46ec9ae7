// Native Llama text-generation engine: C ABI (libcake_engine.so).
//
// The whole text path of one all-local model without Python: checkpoint (safetensors,
// HF names) -> device weights, MFMA-GEMM prefill, hipGraph-captured decode steps
// (hipStreamBeginCapture over the gfx950 kernels' C entry points), device token
// selection, and the per-token replay loop (graph_loop.cpp).  Reference: the master's
// generation loop cake-core/src/cake/master.rs:80-124 and the Llama generator
// cake-core/src/models/llama3/llama.rs:72-138, 277-341.
#pragma once
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef int32_t (*cake_engine_token_cb)(void* ctx, int32_t token);  // non-zero = stop

// CakeEngineOpts.weight_fmt = weight format | CAKE_PREFILL_FMT(prefill_fmt)
#define CAKE_PREFILL_FMT_SHIFT 8
#define CAKE_PREFILL_FMT(p) ((int32_t)((uint32_t)(p) << CAKE_PREFILL_FMT_SHIFT))
#define CAKE_WEIGHT_FMT_OF(w) ((int32_t)((uint32_t)(w) & 0xffu))
#define CAKE_PREFILL_FMT_OF(w) ((int32_t)((uint32_t)(w) >> CAKE_PREFILL_FMT_SHIFT))

struct CakeEngineOpts {
  int32_t max_seq;          // KV-cache length (prompt + generated tokens)
  int32_t dtype;            // 0 = bf16, 1 = f16
  int32_t device;           // GPU ordinal
  int32_t steps_per_graph;  // decode steps per graph replay (greedy only; >= 1)
  int32_t init;             // 0: the checkpoint's safetensors; 1: seeded random-normal
                            // weights of the config.json architecture (benchmarks)
  int32_t weight_fmt;       // 0: projections in the model dtype; 1: FP8 e4m3fn weight-only
                            // projections (q|k|v, o, gate|up, down: one byte per element
                            // + one f32 scale per row), quantised on load; the embedding,
                            // lm_head, norms and KV cache stay 16-bit; 2: OCP MXFP4
                            // weight-only projections (the same four: two e2m1 codes per
                            // byte + one e8m0 scale byte per 32 elements of a row; widths
                            // divisible by 32), quantised on load.  1, 2: not with open_tp.
                            // Bits 8 and up of this word are prefill_fmt (the struct's 40
                            // bytes are full and its layout is fixed; CAKE_PREFILL_FMT below):
                            // 0: prefill runs the weights' own path (weight_fmt 1, 2: each
                            // projection widened into a 16-bit scratch before a 16-bit MFMA
                            // GEMM).  1: FP8 MFMA prefill — every projection quantises its
                            // activation rows per token (e4m3fn codes, scale = amax / 448) and
                            // multiplies them with the resident e4m3fn projection codes on the
                            // fp8 matrix instruction, f32 accumulation, both scales applied to
                            // the finished sum; no dequantise pass.  Requires weight_fmt 1 and
                            // hidden, attention and intermediate widths divisible by 128.
                            // Decode, lm_head and the KV format are unchanged; composes with
                            // head_fmt / kv_fmt; each pipeline rank's or worker's own value
                            // governs its own layers.  Not with open_tp.
  uint64_t seed;            // init = 1: weight seed
  int32_t head_fmt;         // 0: lm_head in the model dtype; 1: e4m3fn codes + one f32 scale per
                            // vocabulary row; 2: MXFP4 (hidden width divisible by 32).  Chosen
                            // independently of weight_fmt; quantised on load with the
                            // projections' row quantisers.  The embedding stays 16-bit (tied:
                            // the quantised head is an extra allocation).  Ranks and workers
                            // without the head ignore it.  1, 2: not with open_tp.
  int32_t kv_fmt;           // 0: KV cache in the model dtype; 1: FP8 e4m3fn KV cache, one code
                            // per element and no scale (code = rne_e4m3(clamp(x, -448, 448)) of
                            // the f32 value the writer holds), half the bytes; every attention
                            // read, prefill included, sees the quantised values.  2: the test
                            // oracle of 1 only — the 16-bit cache and its readers, every writer
                            // storing the code's value (exact in bf16 and f16); it saves no
                            // memory and an engine opened with 1 must equal it bit for bit.
                            // Chosen independently of weight_fmt / head_fmt; each pipeline
                            // rank's or worker's own value governs its own caches.  1, 2: not
                            // with open_tp, not with the experimental decode launches.
};

// Layer-sharded pipeline over one process per GPU.  Placement: `owners[l]` is the rank
// running layer l (a topology: node i -> rank i + 1, unplaced layers on rank 0), any
// pattern — every maximal run of consecutive layers on one rank is one stop of the
// token's walk (llama.rs:95-114); no owner map = contiguous shards, rank 0 lighter by
// the head.  Rank 0 always holds the embedding and the head.  Each decode step's
// hidden state moves between stops by device-side hops (hop.hip, one IPC-mapped inbox
// per edge of the walk: no host in the step), prefill rows through IPC-mapped buffers;
// the control plane (IPC handles, prefill relay, replay announcements) is TCP to rank 0
// at master_addr.  Every edge is self-tested with a tagged pattern at start-up.
struct CakePipeOpts {
  int32_t rank, world;
  const char* master_addr;   // "host:port" rank 0 listens on
  int32_t hop_bf16;          // 1: bf16 hop payload (half the bytes)
  double hop_timeout_s;      // a hop receive that waits longer sets the error word
  double connect_timeout_s;  // workers: how long to retry reaching rank 0
  const int32_t* owners;     // [n_owners == num_hidden_layers] or null
  int32_t n_owners;
};

// Tensor parallel over one process per GPU: every rank holds 1/world of every layer (its
// query / KV heads, its slice of the intermediate rows) and of the vocabulary; the
// decode step's two all-reduces per layer and the token selection are device-side
// (allreduce.hip, IPC-mapped inboxes) inside each rank's captured graph; prefill sums go
// through IPC-mapped slabs.  Rank 0 generates; the others serve (cake_engine_serve).
struct CakeTPOpts {
  int32_t rank, world;       // world <= 8
  const char* master_addr;   // "host:port" rank 0 listens on
  double timeout_s;          // all-reduce wait bound (error word instead of a hang)
  double connect_timeout_s;
};

// Master over TCP workers (the reference's Client, cake-core/src/cake/client.rs:23-133):
// layer l runs on worker worker_of[l] ("host:port", a topology node's host) or locally
// (-1).  One connection per worker (Hello -> WorkerInfo at open); every contiguous run of
// one worker's layers is one Batch round trip per token (llama.rs:95-114), the hidden
// rows travel as f32 tensors.  The decode step runs eagerly (a host round trip sits
// inside it); local runs, the head and the token choice are the same kernels.
struct CakeRemoteOpts {
  const int32_t* worker_of;     // [n_layers == num_hidden_layers]
  int32_t n_layers;
  const char* const* workers;   // [n_workers] "host:port"
  int32_t n_workers;
  double timeout_s;             // connect / reply wait bound
};

struct CakeEngineSampling {
  float temperature;        // <= 0: greedy
  int32_t top_k;            // 0: off
  float top_p;              // 0 or >= 1: off
  uint64_t seed;
  float repeat_penalty;     // 1: off
  int32_t repeat_last_n;
};

// Per-request logit controls (cake_engine_set_logit_controls): OpenAI's presence_penalty /
// frequency_penalty / logit_bias and the min_p truncation rule.
struct CakeLogitControls {
  float presence_penalty;   // [-2, 2]; 0: off
  float frequency_penalty;  // [-2, 2]; 0: off
  float min_p;              // (0, 1]: on for sampled decoding; 0: off; greedy ignores it
  int32_t n_bias;           // <= 300
  const int32_t* bias_ids;  // [n_bias] distinct ids in [0, V)
  const float* bias_values; // [n_bias] finite, in [-100, 100]
};

struct CakeEngineStats {
  int32_t n_prompt;
  int32_t n_generated;
  double prefill_s;         // embed + layers + head + first token (host wall)
  double decode_s;          // generated tokens after the first (host wall)
  double tokens_per_s;      // (n_generated - 1) / decode_s: the reference's rate
  float p50_ms, p99_ms;     // device time per decode token
};

// config.json + safetensors of `model_dir`; null on failure (message in err).
void* cake_engine_open(const char* model_dir, const struct CakeEngineOpts* opts, char* err,
                       int32_t errlen);
// Pipeline rank (see CakePipeOpts): loads only its layer shard, joins the ring.
void* cake_engine_open_pp(const char* model_dir, const struct CakeEngineOpts* opts,
                          const struct CakePipeOpts* pipe, char* err, int32_t errlen);
// Tensor-parallel rank (see CakeTPOpts).
void* cake_engine_open_tp(const char* model_dir, const struct CakeEngineOpts* opts,
                          const struct CakeTPOpts* tp, char* err, int32_t errlen);
// Master with TCP workers (see CakeRemoteOpts): embedding, head and the local layers here.
void* cake_engine_open_remote(const char* model_dir, const struct CakeEngineOpts* opts,
                              const struct CakeRemoteOpts* remote, char* err, int32_t errlen);
// Workers (rank > 0): serve rank 0's control messages until it closes; 0 or an error.
int32_t cake_engine_serve(void* engine, char* err, int32_t errlen);
// TCP worker (topology node): only `layers` (global indices), no embedding / head.
void* cake_engine_open_layers(const char* model_dir, const struct CakeEngineOpts* opts,
                              const int32_t* layers, int32_t n_layers, char* err,
                              int32_t errlen);
// Run `layers` over hidden [T, H] f32 (host memory, in place) at positions pos0.. with
// the KV cache of `session` (created on first use); 0 or an error.
int32_t cake_engine_forward(void* engine, uint64_t session, const int32_t* layers,
                            int32_t n_layers, int32_t pos0, float* hidden, int32_t T, char* err,
                            int32_t errlen);
void cake_engine_drop_session(void* engine, uint64_t session);
// [rank, world, first layer, end layer]
int32_t cake_engine_rank_info(void* engine, int32_t* out4);
// [V, H, L, nh, nkv, hd, I, max_seq]
int32_t cake_engine_info(void* engine, int32_t* out8);
// EOS ids of the config (up to cap); returns the count
int32_t cake_engine_eos(void* engine, int32_t* out, int32_t cap);
// bytes of this rank's device weight allocations: embedding, head if untied, norms,
// projections and their scales (weight_fmt 1: f32 per row; 2: one byte per 32 elements),
// the quantised head and its scales (head_fmt 1, 2: also when the embeddings are tied)
int64_t cake_engine_weight_bytes(void* engine);
// bytes of the packed (lossless 13-bit) copies of bf16 projections / lm_head this rank keeps
// beside the weights for its decode GEMVs (CAKE_PACK16, docs/ENV.md); not in weight_bytes
int64_t cake_engine_packed_bytes(void* engine);
// bytes of one session's K + V cache allocation on this rank:
// 2 * local layers * nkv * max_seq * hd * (kv_fmt 1 ? 1 : 2)
int64_t cake_engine_kv_bytes(void* engine);
// Prefill `prompt` from position 0, then generate up to max_new tokens (the first comes
// from the prefill logits), stopping after an EOS id.  Tokens go to out[] (and cb).
// Returns 0 or an error code (message in err).
int32_t cake_engine_generate(void* engine, const int32_t* prompt, int32_t n_prompt,
                             int32_t max_new, const struct CakeEngineSampling* sampling,
                             const int32_t* eos, int32_t n_eos, cake_engine_token_cb cb,
                             void* ctx, int32_t* out, int32_t out_cap,
                             struct CakeEngineStats* stats, char* err, int32_t errlen);
// Lock-step batched decode of n_seq prompts, 1 <= n_seq <= 8: prompt b is
// tokens[offsets[b], offsets[b + 1]) (offsets: n_seq + 1 entries).  Each prompt is prefilled
// into a KV cache of its own (identical prompts once), the first tokens come from the prefill
// logits, then every step decodes all sequences on one pass over the weights.  One sampling
// setting; sequence b draws with seed + b.  A sequence's tokens are bit for bit those of the
// same prompt decoded alone through this call (with seed + b), whatever else rides in the
// batch.  out[b * max_new + i]: token i of sequence b, out_len[b] of them (its EOS inclusive;
// a sequence that ended keeps its row until all have ended or max_new is reached).
// seq_stats [n_seq] or null (per sequence: n_prompt, n_generated, its rate; the times are the
// call's); stats or null (sums, tokens_per_s of all sequences together, p50 / p99 device ms
// per step).  logits_out: null, or f32 [n_seq, max_new, V] for the rows token selection saw
// (tests; rows at and past out_len[b] are unspecified).  cake_engine_open with weight_fmt 0,
// head_fmt 0 and kv_fmt 0 only; refused (message in err) before any launch: pipeline,
// tensor-parallel, remote and layers-only engines, quantised weights / head / KV cache,
// logprobs or logit controls turned on, n_seq outside 1..8, an empty prompt,
// n_prompt + max_new > max_seq.  Leaves cake_engine_generate / continue state untouched.
int32_t cake_engine_generate_batch(void* engine, const int32_t* tokens, const int32_t* offsets,
                                   int32_t n_seq, int32_t max_new,
                                   const struct CakeEngineSampling* sampling, const int32_t* eos,
                                   int32_t n_eos, int32_t* out, int32_t* out_len,
                                   struct CakeEngineStats* seq_stats, struct CakeEngineStats* stats,
                                   float* logits_out, char* err, int32_t errlen);
// Continue the last generation for up to max_new more tokens (same sampling, the device
// state where the previous generate / continue left it, EOS included): chat turns that
// extend a context, and benchmarks that time exactly max_new decode steps.
int32_t cake_engine_continue(void* engine, int32_t max_new, const int32_t* eos, int32_t n_eos,
                             cake_engine_token_cb cb, void* ctx, int32_t* out, int32_t out_cap,
                             struct CakeEngineStats* stats, char* err, int32_t errlen);
// Teacher forcing (tests): prefill `prompt`, then one decode step per forced token (the
// decode kernels, hops and all-reduces, launched eagerly); out[(n_forced + 1) x V] = the
// f32 logits after the prompt and after each forced token.  Rank 0 of any mode.
int32_t cake_engine_forced_logits(void* engine, const int32_t* prompt, int32_t n_prompt,
                                  const int32_t* forced, int32_t n_forced, float* out, char* err,
                                  int32_t errlen);
// Teacher-forced scoring of tokens[0, n), 2 <= n <= max_seq: one prefill, then the head over
// every row in vocabulary chunks reduced on the device ([n, V] logits never exist).  Row i is
// the distribution after tokens[0..i]: lse[i] = log sum exp of its logits, tgt[i] the logit of
// tokens[i + 1] (NaN on the last row), top[i] / topv[i] the argmax id (lowest at ties) and its
// logit; log p(tokens[i + 1]) = tgt[i] - lse[i].  vchunk: chunk width in vocabulary ids, a
// positive multiple of 256 (clamped to V), or 0 = the largest that keeps the f32 chunk within
// 64 MB.  An engine that holds the head, not tensor parallel; any weight / head / KV /
// prefill format.  Leaves the engine as cake_engine_prefill_logits does.
int32_t cake_engine_score(void* engine, const int32_t* tokens, int32_t n, int32_t vchunk,
                          float* lse, float* tgt, int32_t* top, float* topv, char* err,
                          int32_t errlen);
// Log-probs of generated tokens.  top_k < 0: off (the default); 0..20: on, with that many
// alternatives per token.  Takes effect at the next cake_engine_generate; a continue keeps
// the setting of the generation it continues.  Per token, one launch inside the decode step
// reads the f32 row token selection saw (after the repeat penalty, before temperature /
// top-k / top-p / the draw) and writes a 192-byte record that the read-back ring carries to
// the host with the token.  Refused: a tensor-parallel engine, an engine without the head,
// top_k > 20.  The device buffers are allocated at the first call that turns it on.
int32_t cake_engine_set_logprobs(void* engine, int32_t top_k, char* err, int32_t errlen);
// Records of tokens [first, first + count) of the last generate / continue call (inside the
// token callback: any token reported so far, the current one included): ids[count],
// logit[count] = x[id] bit for bit, lse[count] = log sum exp x (f32; the caller forms
// logprob = (double)logit - (double)lse), top_ids / top_logits [count, 20]: the top_k largest
// logits, descending, the lower id first at ties; entries past min(top_k, V): id -1, -inf.
int32_t cake_engine_logprobs(void* engine, int32_t first, int32_t count, int32_t* ids,
                             float* logit, float* lse, int32_t* top_ids, float* top_logits,
                             char* err, int32_t errlen);
// Logit controls of the generations that follow (null: off, the default).  They act on the f32
// row token selection sees, after the repeat penalty and before argmax / top-k / top-p / the
// draw / the log-prob record, in one launch inside the decode step (kernels/logit_controls.hip):
// with c[v] the occurrences of v among the tokens this generation has produced so far (the
// prompt is not counted; a continue goes on counting), x[v] -= presence + frequency * c[v] where
// c[v] > 0; then x[id] += b for every bias entry; then, for sampled decoding with min_p on, the
// sampling set is cut to x[v] >= max x + T ln(min_p) and intersected with top-k / top-p.  Every
// operation is one f32 rounding (ops/reference.py logit_controls_ref is bit-exact).  Takes
// effect at the next cake_engine_generate; a continue keeps the setting of the generation it
// continues.  All-neutral values (no penalty, no bias, min_p 0) are the same as null: the
// default decode path.  Validated here: ranges, n_bias, distinct ids below V.  Refused: a
// tensor-parallel engine, an engine without the head.  The count table and the parameter block
// are allocated at the first call that turns the controls on.
int32_t cake_engine_set_logit_controls(void* engine, const struct CakeLogitControls* c, char* err,
                                       int32_t errlen);
// "rank:first-last,..." layer runs of the token's walk (placement check); bytes written.
int32_t cake_engine_walk(void* engine, char* out, int32_t cap);
// Logits of the last prompt position after a prefill only (f32 [V] to host), for tests.
int32_t cake_engine_prefill_logits(void* engine, const int32_t* prompt, int32_t n_prompt,
                                   float* out, char* err, int32_t errlen);
void cake_engine_close(void* engine);

#ifdef __cplusplus
}
#endif
