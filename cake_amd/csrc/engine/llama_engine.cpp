// Native Llama engine (see llama_engine.h): host orchestration in C++ over the gfx950
// kernels' C entry points — what models/llama3/{blocks,model}.py + decode_loop.py do
// through PyTorch, with no interpreter, no torch allocator and no torch graphs:
//
//   * weights: HF safetensors (mmap, csrc/runtime/safetensors.cpp) uploaded once into
//     hipMalloc'd buffers in the model dtype (bf16 / f16; other checkpoint dtypes
//     converted on the device by cake_cast16).  q|k|v rows and gate|up rows are packed
//     into one matrix each: the prefill GEMMs read them as one operand, the decode
//     GEMVs take the three / two row blocks as separate pointers.
//   * prefill: embed -> per layer RMSNorm, q|k|v GEMM, RoPE + KV write, causal flash
//     attention, o_proj GEMM (+residual epilogue), RMSNorm, gate|up GEMM (SwiGLU
//     epilogue), down GEMM (+residual) -> final-norm lm_head GEMV on the last row
//     (reference: llama.rs:72-138, transformer.rs:51-73).  GEMM tiles come from the
//     same cost model + measured table (ops/gemm_tuned.json) as ops/gemm.py.
//   * decode: one step = 5 launches per layer + the head; captured with
//     hipStreamBeginCapture into one graph per attention split-cap bucket (the live
//     length picks the bucket), replayed by the native loop (graph_loop.cpp).  Greedy
//     steps end in the fused head_select launch (lm_head + penalty + argmax + the next
//     step's embedding row); sampled steps in threshold + Gumbel-max draws keyed by
//     (seed, step) — the same kernels and launch order as DeviceDecoder, so tokens match
//     the Python engine exactly (tests/test_engine_gpu.py).
#include "llama_engine.h"

#include <dlfcn.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <functional>
#include <list>
#include <map>
#include <memory>
#include <sstream>
#include <stdexcept>
#include <string>
#include <tuple>
#include <vector>

#include "../driver/graph_loop.h"
#include "../kernels/cake_kernels.h"
#include "../runtime/json.h"
#include "../runtime/net.h"
#include "../runtime/proto.h"
#include "../runtime/safetensors.h"
#include "engine_util.h"
#include "llama_weights.h"

namespace cake {
namespace {

// Entry points of csrc/experimental/attn_oproj.hip, found in the loaded kernel library
// (the one that holds cake_attn_decode) when it was built with CAKE_BUILD_EXPERIMENTAL=1;
// all null otherwise.
struct AoFns {
  decltype(&cake_attn_oproj_supported) supported = nullptr;
  decltype(&cake_attn_oproj_ws_floats) ws_floats = nullptr;
  decltype(&cake_attn_oproj_ticket_words) ticket_words = nullptr;
  decltype(&cake_attn_oproj) run = nullptr;
};

AoFns ao_fns() {
  AoFns f;
  Dl_info info;
  if (!dladdr(reinterpret_cast<void*>(&cake_attn_decode), &info) || !info.dli_fname) return f;
  void* h = dlopen(info.dli_fname, RTLD_LAZY | RTLD_NOLOAD);
  if (!h) return f;
  f.supported = reinterpret_cast<decltype(f.supported)>(dlsym(h, "cake_attn_oproj_supported"));
  f.ws_floats = reinterpret_cast<decltype(f.ws_floats)>(dlsym(h, "cake_attn_oproj_ws_floats"));
  f.ticket_words =
      reinterpret_cast<decltype(f.ticket_words)>(dlsym(h, "cake_attn_oproj_ticket_words"));
  f.run = reinterpret_cast<decltype(f.run)>(dlsym(h, "cake_attn_oproj"));
  if (!f.supported || !f.ws_floats || !f.ticket_words || !f.run) f = AoFns{};
  return f;
}


// ---------------------------------------------------------------------------
// model config (config.json; models/llama3/config.py from_dict)
// ---------------------------------------------------------------------------
struct Cfg {
  int H = 0, I = 0, V = 0, L = 0, nh = 0, nkv = 0, hd = 0;
  double eps = 1e-5, theta = 10000.0;
  bool tie = false;
  std::vector<int> eos;
  Json rope_scaling;

  static Cfg parse(const Json& d) {
    auto num = [&](const char* k, double def) {
      return d.has(k) && d.get(k).is_number() ? d.get(k).as_double() : def;
    };
    Cfg c;
    c.H = (int)d.get("hidden_size").as_int();
    c.I = (int)d.get("intermediate_size").as_int();
    c.V = (int)d.get("vocab_size").as_int();
    c.L = (int)d.get("num_hidden_layers").as_int();
    c.nh = (int)d.get("num_attention_heads").as_int();
    c.nkv = d.has("num_key_value_heads") && d.get("num_key_value_heads").is_number()
                ? (int)d.get("num_key_value_heads").as_int() : c.nh;
    c.hd = c.H / c.nh;
    c.eps = num("rms_norm_eps", 1e-5);
    c.theta = num("rope_theta", 10000.0);
    c.tie = d.has("tie_word_embeddings") && d.get("tie_word_embeddings").type() == Json::Bool &&
            d.get("tie_word_embeddings").as_bool();
    if (d.has("eos_token_id")) {
      const Json& e = d.get("eos_token_id");
      if (e.is_array()) {
        for (const auto& x : e.items()) c.eos.push_back((int)x.as_int());
      } else if (e.is_number()) {
        c.eos.push_back((int)e.as_int());
      }
    }
    if (d.has("rope_scaling")) c.rope_scaling = d.get("rope_scaling");
    return c;
  }

  // theta_i = 1 / theta^(2i/d) with optional Llama-3.1 "llama3" scaling (f64, as
  // ops/reference.py inv_freq)
  std::vector<float> inv_freq() const {
    std::vector<float> out(hd / 2);
    const bool l3 = rope_scaling.is_object() &&
                    ((rope_scaling.has("rope_type") && rope_scaling.get("rope_type").is_string() &&
                      rope_scaling.get("rope_type").as_string() == "llama3") ||
                     (rope_scaling.has("type") && rope_scaling.get("type").is_string() &&
                      rope_scaling.get("type").as_string() == "llama3"));
    auto rs = [&](const char* k, double def) {
      return rope_scaling.has(k) && rope_scaling.get(k).is_number() ? rope_scaling.get(k).as_double()
                                                                    : def;
    };
    for (int i = 0; i < hd / 2; ++i) {
      double f = 1.0 / std::pow(theta, (double)(2 * i) / (double)hd);
      if (l3) {
        const double factor = rs("factor", 8.0), lo = rs("low_freq_factor", 1.0),
                     hi = rs("high_freq_factor", 4.0),
                     old = rs("original_max_position_embeddings", 8192.0);
        const double lo_wl = old / lo, hi_wl = old / hi, wl = 2.0 * M_PI / f;
        const double o = wl > lo_wl ? f / factor : f;
        const double smooth = (old / wl - lo) / (hi - lo);
        const double mid = (1.0 - smooth) * o / factor + smooth * o;
        f = (wl >= hi_wl && wl <= lo_wl) ? mid : o;
      }
      out[i] = (float)f;
    }
    return out;
  }
};


// Contiguous layer shards, rank 0 lighter by the head's weight in blocks
// (parallel/pipeline.py shard_layers + head_cost_in_layers).
std::vector<std::pair<int, int>> shard_layers(const Cfg& c, int world) {
  std::vector<std::pair<int, int>> out;
  if (world <= 1) {
    out.push_back({0, c.L});
    return out;
  }
  if (world > c.L) {  // one layer per rank, the ranks past the last layer idle
    for (int r = 0; r < world; ++r) out.push_back(r < c.L ? std::make_pair(r, r + 1)
                                                          : std::make_pair(c.L, c.L));
    return out;
  }
  const double layer_bytes = 2.0 * ((double)c.H * (c.nh + 2 * c.nkv) * c.hd +
                                    (double)c.nh * c.hd * c.H + 3.0 * c.H * c.I + 2.0 * c.H);
  const double head = 2.0 * (double)c.V * c.H / layer_bytes;
  const double total = c.L + head;
  int start = 0;
  for (int r = 0; r < world; ++r) {
    int end = r < world - 1 ? (int)std::nearbyint((r + 1) * total / world - head) : c.L;
    end = std::max(start + (c.L - start >= world - r ? 1 : 0), std::min(end, c.L - (world - 1 - r)));
    out.push_back({start, end});
    start = end;
  }
  return out;
}

// [start, end) of rank's contiguous share of n items (parallel/tensor_parallel.py)
std::pair<int, int> split_range(int n, int world, int rank) {
  const int q = n / world, r = n % world;
  const int a = rank * q + std::min(rank, r);
  return {a, a + q + (rank < r ? 1 : 0)};
}

// CAKE_ENGINE_TRACE=1: control-plane progress on stderr (rank-tagged, seconds since the
// process's first trace line) — where a multi-rank start or generation stands
bool trace_on() {
  static const bool on = [] {
    const char* v = std::getenv("CAKE_ENGINE_TRACE");
    return v && *v && std::string(v) != "0";
  }();
  return on;
}
void trace(int rank, const std::string& what) {
  if (!trace_on()) return;
  static const auto t0 = std::chrono::steady_clock::now();
  const double t = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  std::fprintf(stderr, "[engine r%d +%.3fs] %s\n", rank, t, what.c_str());
  std::fflush(stderr);
}

// refused before any network or GPU work, so a caller can never hang on it
const char* const kNoFp8TP =
    "fp8 weights (weight_fmt 1) are not supported with tensor parallelism yet: open the "
    "tensor-parallel engine with weight_fmt 0";

const char* const kNoQHeadTP =
    "a quantised lm_head (head_fmt 1 = fp8, 2 = mxfp4) is not supported with tensor "
    "parallelism: open the tensor-parallel engine with head_fmt 0";

const char* const kNoKvTP =
    "a quantised KV cache (kv_fmt 1 = fp8, 2 = its 16-bit oracle) is not supported with tensor "
    "parallelism: open the tensor-parallel engine with kv_fmt 0";

const char* const kNoPrefillTP =
    "an fp8 MFMA prefill (prefill_fmt 1) is not supported with tensor parallelism: open the "
    "tensor-parallel engine with prefill_fmt 0";

Json msg(const char* cmd) {
  Json j = Json::object();
  j.set("cmd", Json::string(cmd));
  return j;
}

// the decode GEMV kinds that read a packed (13-bit) copy of their bf16 weights by default:
// those whose in-graph kernel time, at the best tuning found, fell below the 16-bit twin's by
// more than the run-to-run spread in the 8B decode graph: gate | up, down_proj and the
// lm_head; q | k | v and o_proj were not faster at any tuning tried.  The
// figures of every kind, adopted or not, are in profiles/pack13_decode_tuning_sweep.jsonl and
// profiles/pack13_decode8b_kernel_table.txt; a kind that is not adopted gets no copy.
// CAKE_PACK16_KINDS overrides (qkv, o, gu, down, head).
static const char* const kPack13Kinds = "gu,down,head";

// ---------------------------------------------------------------------------
// the engine
// ---------------------------------------------------------------------------
class Llama {
 public:
  Llama(const std::string& dir, const CakeEngineOpts& o, const CakePipeOpts* pp = nullptr,
        const std::vector<int>* layers = nullptr, const CakeTPOpts* tp = nullptr,
        const CakeRemoteOpts* remote = nullptr)
      : dt_(o.dtype), dev_(o.device), init_(o.init), wfmt_(CAKE_WEIGHT_FMT_OF(o.weight_fmt)),
        hfmt_(o.head_fmt), kvfmt_(o.kv_fmt), pfmt_(CAKE_PREFILL_FMT_OF(o.weight_fmt)),
        seed_(o.seed) {
    if (dt_ != 0 && dt_ != 1) throw Error("dtype must be 0 (bf16) or 1 (f16)");
    if (wfmt_ != 0 && wfmt_ != 1 && wfmt_ != 2)
      throw Error("weight_fmt must be 0 (model dtype), 1 (fp8 e4m3 projections) or 2 (mxfp4 "
                  "projections)");
    if (wfmt_ != 0 && tp) throw Error(kNoFp8TP);
    if (hfmt_ != 0 && hfmt_ != 1 && hfmt_ != 2)
      throw Error("head_fmt must be 0 (model dtype), 1 (fp8 e4m3 lm_head) or 2 (mxfp4 lm_head)");
    if (hfmt_ != 0 && tp) throw Error(kNoQHeadTP);
    if (kvfmt_ != kKv16 && kvfmt_ != kKvFp8 && kvfmt_ != kKvFp8Emu)
      throw Error("kv_fmt must be 0 (model dtype), 1 (fp8 e4m3 KV cache) or 2 (fp8 values in a "
                  "16-bit cache: the test oracle)");
    if (kvfmt_ != kKv16 && tp) throw Error(kNoKvTP);
    if (kvfmt_ != kKv16) {
      // the fp8 cache has core 2's split launch only: none of the experimental decode
      // paths (docs/ENV.md) reads it
      for (const char* name : {"CAKE_ATTN_OPROJ", "CAKE_ATTN_HEADS", "CAKE_MK", "CAKE_QKV_ATTN"}) {
        const char* e = std::getenv(name);
        if (e && *e && std::string(e) != "0")
          throw Error(std::string("a quantised KV cache (kv_fmt ") + std::to_string(kvfmt_) +
                      ") does not run the experimental decode path " + name + "=" + e +
                      ": unset it or open with kv_fmt 0");
      }
    }
    if (pfmt_ != 0 && pfmt_ != 1)
      throw Error("prefill_fmt must be 0 (the weights' prefill) or 1 (fp8 MFMA prefill with "
                  "per-token e4m3 activations)");
    if (pfmt_ != 0 && tp) throw Error(kNoPrefillTP);
    if (pfmt_ == 1 && wfmt_ != 1)
      throw Error("an fp8 MFMA prefill (prefill_fmt 1) runs on the resident fp8 projection codes: "
                  "open with weight_fmt 1 (fp8), not " + std::to_string(wfmt_));
    if (init_ != 0 && init_ != 1) throw Error("init must be 0 (checkpoint) or 1 (random)");
    if (tp) {
      tp_ = tp->world;
      tp_rank_ = tp->rank;
      hop_timeout_ = tp->timeout_s > 0 ? tp->timeout_s : 30.0;
      if (tp_ < 1 || tp_ > 8 || tp_rank_ < 0 || tp_rank_ >= tp_) throw Error("bad TP rank / world");
      int n = 0;
      hip_check(hipGetDeviceCount(&n), "hipGetDeviceCount");
      if (n > 0) dev_ %= n;
    }
    if (pp) {
      rank_ = pp->rank;
      world_ = pp->world;
      hop_bf16_ = pp->hop_bf16 != 0;
      hop_timeout_ = pp->hop_timeout_s > 0 ? pp->hop_timeout_s : 30.0;
      if (world_ < 1 || rank_ < 0 || rank_ >= world_) throw Error("bad rank / world");
      // one process per GPU; more ranks than GPUs share them round-robin (rehearsals on
      // a one-GPU box, as parallel/pipeline_bench.py DistEnv)
      int n = 0;
      hip_check(hipGetDeviceCount(&n), "hipGetDeviceCount");
      if (n > 0) dev_ %= n;
    }
    hip_check(hipSetDevice(dev_), "hipSetDevice");
    hip_check(hipStreamCreateWithFlags(&st_, hipStreamNonBlocking), "hipStreamCreate");
    cfg_ = Cfg::parse(Json::parse(read_file(dir + "/config.json")));
    S_ = o.max_seq > 0 ? o.max_seq : 4096;
    k_ = std::max(1, o.steps_per_graph);
    if (cfg_.H % 8 || cfg_.hd % 2 || cfg_.nh % cfg_.nkv) throw Error("unsupported model shape");
    if (kvfmt_ != kKv16 && cfg_.hd != 64 && cfg_.hd != 128)
      throw Error("an fp8 KV cache needs a head dimension of 64 or 128");
    // this rank's compute shapes: the whole model, or its tensor-parallel slice
    lc_ = cfg_;
    if (tp_ > 1) {
      if (cfg_.nh % tp_ || cfg_.nkv % tp_)
        throw Error("tensor-parallel degree must divide the query and KV heads");
      lc_.nh = cfg_.nh / tp_;
      lc_.nkv = cfg_.nkv / tp_;
      const auto ir = split_range(cfg_.I, tp_, tp_rank_);
      const auto vr = split_range(cfg_.V, tp_, tp_rank_);
      i0_ = ir.first;
      lc_.I = ir.second - ir.first;
      voff_ = vr.first;
      lc_.V = vr.second - vr.first;
      if (lc_.I % 8 || (lc_.nh * cfg_.hd) % 8) throw Error("tensor-parallel slice not 8-aligned");
    }
    const FmtFacts& wf = fmt_facts(wfmt_);
    if (cfg_.H % wf.multiple || (cfg_.nh * cfg_.hd) % wf.multiple || cfg_.I % wf.multiple)
      throw Error(std::string(wf.name) + " weights need hidden, attention and intermediate "
                  "widths divisible by " + std::to_string(wf.multiple));
    if (pfmt_ == 1 && (cfg_.H % 128 || (cfg_.nh * cfg_.hd) % 128 || cfg_.I % 128))
      throw Error("an fp8 MFMA prefill needs hidden, attention and intermediate widths divisible "
                  "by 128 (the k of one MFMA step)");
    if (layers) {  // a TCP worker: the topology node's layers, no embedding / head
      hfmt_ = 0;   // no head here: the option is accepted and ignored
      owned_ = *layers;
      std::sort(owned_.begin(), owned_.end());
      owned_.erase(std::unique(owned_.begin(), owned_.end()), owned_.end());
      if (owned_.empty() || owned_.front() < 0 || owned_.back() >= cfg_.L)
        throw Error("worker layers outside the model");
      head_ = false;
    } else {
      // layer -> rank: the topology's owner map, or contiguous shards
      const bool placed = pp && pp->owners && pp->n_owners > 0;
      owner_.assign(cfg_.L, 0);
      if (placed) {
        if (pp->n_owners != cfg_.L)
          throw Error("owner map has " + std::to_string(pp->n_owners) + " entries for " +
                      std::to_string(cfg_.L) + " layers");
        for (int l = 0; l < cfg_.L; ++l) {
          if (pp->owners[l] < 0 || pp->owners[l] >= world_)
            throw Error("layer " + std::to_string(l) + " placed on rank " +
                        std::to_string(pp->owners[l]) + " outside the world of " +
                        std::to_string(world_));
          owner_[l] = pp->owners[l];
        }
      } else {
        const auto sh = shard_layers(cfg_, world_);
        for (int r = 0; r < world_; ++r)
          for (int l = sh[r].first; l < sh[r].second; ++l) owner_[l] = r;
      }
      if (remote) {  // TCP workers: layer -> worker index, -1 = local
        if (remote->n_layers != cfg_.L || !remote->worker_of)
          throw Error("remote placement must name every layer (-1 = local)");
        remote_of_.assign(remote->worker_of, remote->worker_of + cfg_.L);
        for (int l = 0; l < cfg_.L; ++l)
          if (remote_of_[l] < -1 || remote_of_[l] >= remote->n_workers)
            throw Error("layer " + std::to_string(l) + " placed on an unknown worker");
        for (int w = 0; w < remote->n_workers; ++w)
          remotes_.push_back({remote->workers[w] ? remote->workers[w] : "", -1});
        remote_timeout_ = remote->timeout_s > 0 ? remote->timeout_s : 60.0;
      }
      for (int l = 0; l < cfg_.L; ++l)
        if (owner_[l] == rank_ && (remote_of_.empty() || remote_of_[l] < 0)) owned_.push_back(l);
      head_ = rank_ == 0;
      if (!head_) hfmt_ = 0;  // the head lives on rank 0: accepted and ignored elsewhere
    }
    if (const FmtFacts& hf = fmt_facts(hfmt_); cfg_.H % hf.multiple)
      throw Error(std::string("an ") + hf.name + " lm_head needs a hidden width divisible by " +
                  std::to_string(hf.multiple));
    lo_ = owned_.empty() ? 0 : owned_.front();
    hi_ = owned_.empty() ? 0 : owned_.back() + 1;
    local_.assign(cfg_.L, -1);
    for (size_t i = 0; i < owned_.size(); ++i) local_[owned_[i]] = (int)i;
    if (!layers) plan_walk();
    planner_.load(pkg_dir() + "/ops/gemm_tuned.json");
    load_weights(dir);
    // one line per open: what the weights are and what they occupy
    const std::string dtn = dt_ == 0 ? "bf16" : "f16";
    std::fprintf(stderr,
                 "cake engine: weights %s, lm_head %s, kv cache %s%s, %lld bytes on device (rank %d, "
                 "%d layers)\n",
                 (wfmt_ == kFmt16 ? dtn
                                  : fmt_facts(wfmt_).banner + (" projections (" + dtn + " rest)"))
                     .c_str(),
                 !head_ ? "none" : hfmt_ == kFmt16 ? dtn.c_str() : fmt_facts(hfmt_).banner,
                 kvfmt_ == kKvFp8 ? "fp8 e4m3"
                 : kvfmt_ == kKvFp8Emu ? (dt_ == 0 ? "fp8 e4m3 values in bf16 (test oracle)"
                                                   : "fp8 e4m3 values in f16 (test oracle)")
                                       : (dt_ == 0 ? "bf16" : "f16"),
                 pfmt_ == 1 ? ", prefill fp8 e4m3 activations" : "",
                 (long long)weight_bytes_, rank(), (int)owned_.size());
    alloc_state();
    warm_library();
    pack13_all();  // after the KV cache and the workspaces: it takes what HBM they left
    {
      size_t fr = 0, tot = 0;
      (void)hipMemGetInfo(&fr, &tot);
      trace(rank(), "weights + state ready (" + std::to_string(owned_.size()) + " layers), " +
                        std::to_string(fr >> 20) + " of " + std::to_string(tot >> 20) +
                        " MiB free");
    }
    if (world_ > 1) {
      connect_pipeline(pp->master_addr ? pp->master_addr : "127.0.0.1:29517",
                       pp->connect_timeout_s > 0 ? pp->connect_timeout_s : 600.0);
      trace(rank_, "pipeline connected: walk " + walk_str() + ", " +
                       std::to_string(edges_.size()) + " edges");
      selftest_pipeline();
      trace(rank_, "pipeline self-test passed");
    }
    if (tp_ > 1) {
      connect_tp(tp->master_addr ? tp->master_addr : "127.0.0.1:29517",
                 tp->connect_timeout_s > 0 ? tp->connect_timeout_s : 600.0);
      trace(rank(), "tensor-parallel channels mapped");
      selftest_tp();
      trace(rank(), "tensor-parallel self-test passed");
    }
    if (!remotes_.empty()) connect_remotes();
  }

  ~Llama() {
    (void)hipSetDevice(dev_);
    (void)hipStreamSynchronize(st_);
    if (rank_ == 0 && tp_rank_ == 0)
      for (int r = 1; r <= ctl_.workers(); ++r) {
        try {
          ctl_.send(r, msg("exit"));
        } catch (const std::exception&) {
        }
      }
    ctl_.close();
    for (auto& r : remotes_)
      if (r.fd >= 0) tcp_close(r.fd);
    drop_graphs();
    for (void* p : tp_mapped_) (void)hipIpcCloseMemHandle(p);
    for (void* p : tp_owned_) (void)cake_hop_free(p);
    for (auto& kv : out_inbox_) (void)hipIpcCloseMemHandle(kv.second);
    for (auto& kv : peer_pbuf_) (void)hipIpcCloseMemHandle(kv.second);
    for (auto& kv : my_inbox_) (void)cake_hop_free(kv.second);
    if (relay_) (void)cake_hop_free(relay_);
    if (b_.host_tok) (void)hipHostFree(b_.host_tok);
    for (void* p : allocs_) (void)hipFree(p);
    (void)hipStreamDestroy(st_);
  }

  int rank() const { return tp_ > 1 ? tp_rank_ : rank_; }
  int world() const { return tp_ > 1 ? tp_ : world_; }
  std::pair<int, int> layer_range() const { return {lo_, hi_}; }

  const Cfg& cfg() const { return cfg_; }
  int max_seq() const { return S_; }
  int64_t weight_bytes() const { return weight_bytes_; }
  int64_t packed_bytes() const { return packed_bytes_; }
  int64_t kv_bytes() const { return 2 * (int64_t)kv_elems() * kv_esize(); }

  void prefill_logits(const int32_t* prompt, int T, float* host_logits) {
    hip_check(hipSetDevice(dev_), "hipSetDevice");
    if (!head_) throw Error("prefill_logits() runs on pipeline rank 0");
    prefill(prompt, T);
    hip_check(hipMemcpyAsync(host_logits, logits_, sizeof(float) * cfg_.V, hipMemcpyDeviceToHost,
                             st_), "logits D2H");
    hip_check(hipStreamSynchronize(st_), "sync");
  }

  void forced_logits(const int32_t* prompt, int T, const int32_t* forced, int n, float* out) {
    hip_check(hipSetDevice(dev_), "hipSetDevice");
    if (!head_ || tp_rank_ != 0) throw Error("forced_logits() runs on rank 0");
    if (T <= 0 || n < 0 || T + n + 1 > S_) throw Error("prompt + forced tokens exceed max_seq");
    forced_run(prompt, T, forced, n, out);
  }

  // Teacher-forced scoring of tokens[0, n): one prefill, then the head over every row in
  // vocabulary chunks (a store32 GEMM into an f32 scratch [n, Vc], reduced in place by
  // cake_lse_rows), so [n, V] logits never exist.  Row i: lse, the logit of tokens[i + 1]
  // (NaN on the last row), the argmax id and its logit.  The engine is left as
  // prefill_logits() leaves it.
  void score(const int32_t* tokens, int n, int vchunk, float* lse, float* tgt, int32_t* top,
             float* topv) {
    hip_check(hipSetDevice(dev_), "hipSetDevice");
    if (tp_ > 1)
      throw Error("score() is not available on a tensor-parallel engine (the vocabulary is "
                  "sharded)");
    if (!head_) throw Error("score() runs on an engine that holds the head (pipeline rank 0)");
    const int V = cfg_.V;
    if (n < 2) throw Error("score() needs at least 2 tokens");
    if (n > S_) throw Error("score(): " + std::to_string(n) + " tokens exceed max_seq " +
                            std::to_string(S_));
    for (int i = 0; i < n; ++i)
      if (tokens[i] < 0 || tokens[i] >= V)
        throw Error("score(): token id " + std::to_string(tokens[i]) + " at " +
                    std::to_string(i) + " is outside [0, " + std::to_string(V) + ")");
    int Vc = vchunk;
    if (vchunk == 0) {  // the largest multiple of 256 with n Vc 4 bytes <= 64 MB
      const long long fit = (64LL << 20) / (4LL * n) / 256 * 256;
      Vc = (int)std::max<long long>(256, fit);
    } else if (vchunk < 0 || vchunk % 256) {
      throw Error("score(): vchunk is 0 or a positive multiple of 256, got " +
                  std::to_string(vchunk));
    }
    Vc = std::min(Vc, V);
    grow_score(n, Vc);
    prefill_body(tokens, n);
    const int H = cfg_.H;
    std::vector<int32_t> target(tokens + 1, tokens + n);
    target.push_back(-1);
    hip_check(hipMemcpyAsync(sc_target_, target.data(), sizeof(int32_t) * n,
                             hipMemcpyHostToDevice, st_), "targets H2D");
    k_check(cake_rmsnorm(dt_, hidden_, norm_, (float)cfg_.eps, n, H, x16_, st_), "rmsnorm");
    for (int v0 = 0; v0 < V; v0 += Vc) {
      const int w = std::min(Vc, V - v0);
      const void* rows = dense16(lm_head_, v0, w, sc_head_, dt_, st_);
      gemm(kEpiStore32, x16_, H, rows, H, nullptr, 0, sc_logits_, Vc, n, w, H, "gemm score head");
      k_check(cake_lse_rows(sc_logits_, Vc, n, w, v0, v0 == 0, sc_target_, sc_max_, sc_sum_,
                            sc_tgt_, sc_key_, st_), "lse_rows");
    }
    k_check(cake_lse_finish(sc_max_, sc_sum_, sc_key_, n, sc_lse_, sc_top_, sc_topv_, st_),
            "lse_finish");
    hip_check(hipMemcpyAsync(lse, sc_lse_, sizeof(float) * n, hipMemcpyDeviceToHost, st_), "D2H");
    hip_check(hipMemcpyAsync(tgt, sc_tgt_, sizeof(float) * n, hipMemcpyDeviceToHost, st_), "D2H");
    hip_check(hipMemcpyAsync(top, sc_top_, sizeof(int32_t) * n, hipMemcpyDeviceToHost, st_),
              "D2H");
    hip_check(hipMemcpyAsync(topv, sc_topv_, sizeof(float) * n, hipMemcpyDeviceToHost, st_),
              "D2H");
    hip_check(hipStreamSynchronize(st_), "sync");
    if (world_ > 1) sync_workers(hop_drain());
    check_attn_error("rank " + std::to_string(rank()));
  }

  // Log-probs of the generated tokens, from the next generate() on: top_k < 0 off (the
  // default), 0..20 on with that many alternatives per token.  The record array [max_seq],
  // the partials workspace and the ticket are allocated at the first call that turns it on.
  void set_logprobs(int top_k) {
    hip_check(hipSetDevice(dev_), "hipSetDevice");
    if (top_k > kLpMaxK)
      throw Error("log-probs: at most " + std::to_string(kLpMaxK) +
                  " alternatives per token, got " + std::to_string(top_k));
    if (top_k >= 0 && tp_ > 1)
      throw Error("log-probs are not available on a tensor-parallel engine (the vocabulary is "
                  "sharded)");
    if (top_k >= 0 && !head_)
      throw Error("log-probs need an engine that holds the head (pipeline rank 0)");
    if (top_k >= 0 && !lp_rec_) {
      lp_rec_ = dalloc<uint32_t>((size_t)S_ * kLpRecWords);
      lp_ws_ = dalloc<uint8_t>((size_t)cake_logprob_ws_bytes(lc_.V));
      lp_ticket_ = dalloc<unsigned int>(4);
      hip_check(hipMemsetAsync(lp_rec_, 0, sizeof(uint32_t) * (size_t)S_ * kLpRecWords, st_),
                "memset");
      hip_check(hipMemsetAsync(lp_ticket_, 0, 16, st_), "memset");
      hip_check(hipStreamSynchronize(st_), "sync");
    }
    lp_k_ = top_k < 0 ? -1 : top_k;
  }

  // Records of tokens [first, first + count) of the last generate() / continue() call, from
  // the host copy (inside the token callback: every token reported so far, the current one
  // included).  top_ids / top_logits are [count, 20]; entries past the call's top_k are id -1,
  // logit -inf.
  void logprobs(int first, int count, int32_t* ids, float* logit, float* lse, int32_t* top_ids,
                float* top_logits) const {
    if (!lp_on_) throw Error("the last generation ran without log-probs (set_logprobs)");
    if (first < 0 || count < 0 || first + count > lp_n_)
      throw Error("log-probs of tokens [" + std::to_string(first) + ", " +
                  std::to_string(first + count) + ") asked, " + std::to_string(lp_n_) +
                  " generated");
    for (int i = 0; i < count; ++i) {
      const uint32_t* r = lp_host_.data() + (size_t)(first + i) * kLpRecWords;
      ids[i] = (int32_t)r[0];
      std::memcpy(logit + i, r + 1, 4);
      std::memcpy(lse + i, r + 2, 4);
      std::memcpy(top_ids + (size_t)i * kLpMaxK, r + 4, 4 * kLpMaxK);
      std::memcpy(top_logits + (size_t)i * kLpMaxK, r + 4 + kLpMaxK, 4 * kLpMaxK);
    }
  }

  // Logit controls of the generations that follow (null or all-neutral values: off).  Checked
  // here; the count table [V], the parameter block and the state words are allocated at the
  // first call that turns them on; the device block is written when a generation starts.
  void set_logit_controls(const CakeLogitControls* c) {
    LcSetting n;
    if (c) {
      auto in = [](float v, float lo, float hi) { return v >= lo && v <= hi; };  // NaN: false
      if (!in(c->presence_penalty, -2.f, 2.f))
        throw Error("logit controls: presence_penalty must lie in [-2, 2], got " +
                    std::to_string(c->presence_penalty));
      if (!in(c->frequency_penalty, -2.f, 2.f))
        throw Error("logit controls: frequency_penalty must lie in [-2, 2], got " +
                    std::to_string(c->frequency_penalty));
      if (!in(c->min_p, 0.f, 1.f))
        throw Error("logit controls: min_p must lie in [0, 1] (0: off), got " +
                    std::to_string(c->min_p));
      if (c->n_bias < 0 || c->n_bias > kLcMaxBias)
        throw Error("logit controls: at most " + std::to_string(kLcMaxBias) +
                    " logit_bias entries, got " + std::to_string(c->n_bias));
      if (c->n_bias > 0 && (!c->bias_ids || !c->bias_values))
        throw Error("logit controls: null logit_bias arrays");
      n.ids.assign(c->bias_ids, c->bias_ids + c->n_bias);
      n.vals.assign(c->bias_values, c->bias_values + c->n_bias);
      std::vector<int32_t> sorted = n.ids;
      std::sort(sorted.begin(), sorted.end());
      for (int i = 0; i < c->n_bias; ++i) {
        if (n.ids[i] < 0 || n.ids[i] >= cfg_.V)
          throw Error("logit controls: logit_bias id " + std::to_string(n.ids[i]) +
                      " is outside the vocabulary [0, " + std::to_string(cfg_.V) + ")");
        if (i > 0 && sorted[i] == sorted[i - 1])
          throw Error("logit controls: logit_bias id " + std::to_string(sorted[i]) +
                      " is listed twice");
        if (!in(n.vals[i], -100.f, 100.f))
          throw Error("logit controls: logit_bias values must lie in [-100, 100], got " +
                      std::to_string(n.vals[i]) + " for id " + std::to_string(n.ids[i]));
      }
      n.presence = c->presence_penalty;
      n.frequency = c->frequency_penalty;
      n.min_p = c->min_p;
      n.on = n.presence != 0.f || n.frequency != 0.f || n.min_p > 0.f || c->n_bias > 0;
    }
    if (n.on && tp_ > 1)
      throw Error("logit controls (presence_penalty, frequency_penalty, logit_bias, min_p) are "
                  "not available on a tensor-parallel engine (the vocabulary is sharded)");
    if (n.on && !head_)
      throw Error("logit controls need an engine that holds the head (pipeline rank 0)");
    if (n.on && !lc_cnt_) {
      hip_check(hipSetDevice(dev_), "hipSetDevice");
      lc_cnt_ = dalloc<unsigned int>((size_t)lc_.V);
      lc_params_ = dalloc<unsigned int>(kLcParamWords);
      lc_state_ = dalloc<unsigned int>(kLcStateWords);
      hip_check(hipMemsetAsync(lc_state_, 0, sizeof(unsigned int) * kLcStateWords, st_), "memset");
      hip_check(hipStreamSynchronize(st_), "sync");
    }
    lc_next_ = std::move(n);
  }

  void generate(const int32_t* prompt, int T, int max_new, const CakeEngineSampling& smp,
                const int32_t* eos, int n_eos, cake_engine_token_cb cb, void* ctx, int32_t* out,
                int out_cap, CakeEngineStats* stats) {
    hip_check(hipSetDevice(dev_), "hipSetDevice");
    if (!head_) throw Error("generate() runs on pipeline rank 0");
    if (tp_ > 1 && tp_rank_ != 0) throw Error("generate() runs on tensor-parallel rank 0");
    if (T <= 0) throw Error("empty prompt");
    if (max_new <= 0) return;
    if (T + max_new + k_ + 1 > S_) throw Error("prompt + max_new exceeds max_seq");
    if (out_cap < max_new) throw Error("output buffer smaller than max_new");
    if (tp_ > 1) {  // every tensor-parallel rank runs the same steps: tell them what
      Json m = msg("generate");
      Json pr = Json::array();
      for (int i = 0; i < T; ++i) pr.push(Json::integer(prompt[i]));
      m.set("prompt", pr);
      m.set("max_new", Json::integer(max_new));
      m.set("temperature", Json::number(smp.temperature));
      m.set("top_k", Json::integer(smp.top_k));
      m.set("top_p", Json::number(smp.top_p));
      m.set("seed", Json::string(std::to_string(smp.seed)));
      m.set("penalty", Json::number(smp.repeat_penalty));
      m.set("last_n", Json::integer(smp.repeat_last_n));
      m.set("eos", eos_json(eos, n_eos));
      ctl_.broadcast(m);
    }
    run_generation(prompt, T, max_new, smp, eos, n_eos, cb, ctx, out, out_cap, stats, true);
  }

  // More tokens after the last generate / continue: the device history, position and
  // graphs (same sampling mode) are where that call left them.
  void continue_gen(int max_new, const int32_t* eos, int n_eos, cake_engine_token_cb cb,
                    void* ctx, int32_t* out, int out_cap, CakeEngineStats* stats) {
    hip_check(hipSetDevice(dev_), "hipSetDevice");
    if (!head_) throw Error("continue() runs on pipeline rank 0");
    if (tp_ > 1 && tp_rank_ != 0) throw Error("continue() runs on tensor-parallel rank 0");
    if (!have_graphs_) throw Error("continue() needs a previous generate()");
    if (max_new <= 0) return;
    if (out_cap < max_new) throw Error("output buffer smaller than max_new");
    const int L = read_i32(hist_len_);
    if (L + max_new + k_ + 1 > S_) throw Error("context + max_new exceeds max_seq");
    if (tp_ > 1) {
      Json m = msg("continue");
      m.set("max_new", Json::integer(max_new));
      m.set("eos", eos_json(eos, n_eos));
      ctl_.broadcast(m);
    }
    lp_begin(last_mode_.logprobs >= 0, max_new);
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<float> ms;
    const int n_out = remote_mode()
                          ? decode_eager(L - 1, max_new, last_mode_, eos, n_eos, cb, ctx, out,
                                         out_cap, &ms)
                          : decode_tokens(L, max_new, eos, n_eos, cb, ctx, out, out_cap, true, &ms);
    const auto t1 = std::chrono::steady_clock::now();
    if (stats) {
      fill_stats(stats, L, n_out, 0.0, std::chrono::duration<double>(t1 - t0).count(), ms);
      // every token of a continuation is a decode step: the rate counts all of them
      stats->tokens_per_s = stats->decode_s > 0 ? n_out / stats->decode_s : 0.0;
    }
  }

  // Lock-step batched decode of B <= 8 sequences: each prompt through the ordinary prefill
  // into a KV set of its own (identical prompts once, the live rows copied), the first tokens
  // from the prefill logits, then one step for all rows: embedding, per layer RMSNorm ->
  // cake_gemv_rows (q|k|v, f32) -> cake_rope_kv_rows -> the batch-1 decode attention launch
  // per sequence -> gemv_rows (o_proj into the f32 residual rows) -> RMSNorm -> gemv_rows
  // (SwiGLU) -> gemv_rows (down_proj), the head as gemv_rows over [B, V], and the selection
  // kernels once per sequence on that sequence's own state, sequence b drawing with seed + b.
  // The weights are read once per step, not once per sequence.  Launched eagerly; the host
  // reads the tokens one step behind.  Every row's arithmetic is independent of B and of the
  // row's slot, so a sequence's tokens are those of the same prompt decoded alone.  A sequence
  // that met EOS keeps its row until the others end; nothing more of it is reported.
  // logits_out (tests): [B, max_new, V], the rows token selection saw; rows at and past
  // out_len[b] are unspecified.
  void generate_batch(const int32_t* tokens, const int32_t* offsets, int B, int max_new,
                      const CakeEngineSampling& smp, const int32_t* eos, int n_eos, int32_t* out,
                      int32_t* out_len, CakeEngineStats* seq_stats, CakeEngineStats* stats,
                      float* logits_out) {
    hip_check(hipSetDevice(dev_), "hipSetDevice");
    const char* who = "generate_batch() runs on a single-rank engine with 16-bit weights: not ";
    if (world_ > 1) throw Error(std::string(who) + "on a pipeline engine");
    if (tp_ > 1) throw Error(std::string(who) + "on a tensor-parallel engine");
    if (remote_mode()) throw Error(std::string(who) + "on an engine with remote workers");
    if (!head_ || (int)owned_.size() != cfg_.L)
      throw Error(std::string(who) + "on a layers-only engine");
    if (wfmt_ != kFmt16)
      throw Error(std::string(who) + "with " + fmt_facts(wfmt_).name + " weights (weight_fmt " +
                  std::to_string(wfmt_) + ")");
    if (hfmt_ != kFmt16)
      throw Error(std::string(who) + "with an " + fmt_facts(hfmt_).name + " lm_head (head_fmt " +
                  std::to_string(hfmt_) + ")");
    if (kvfmt_ != kKv16)
      throw Error(std::string(who) + "with a quantised KV cache (kv_fmt " + std::to_string(kvfmt_) +
                  ")");
    if (lp_k_ >= 0) throw Error("generate_batch() does not record logprobs: turn them off first");
    if (lc_next_.on)
      throw Error("generate_batch() does not apply logit controls: turn them off first");
    if (B < 1 || B > kMaxBatch)
      throw Error("generate_batch() takes 1 to " + std::to_string(kMaxBatch) + " prompts, got " +
                  std::to_string(B));
    const Cfg& c = cfg_;
    const int nq = c.nh * c.hd;
    if (c.H % 32 || nq % 32 || c.I % 32 || c.V % 4)
      throw Error("generate_batch() needs hidden, attention and intermediate widths divisible by "
                  "32 and a vocabulary divisible by 4");
    std::vector<int> T(B);
    for (int b = 0; b < B; ++b) {
      T[b] = offsets[b + 1] - offsets[b];
      if (T[b] <= 0) throw Error("generate_batch(): empty prompt (sequence " + std::to_string(b) + ")");
      if (max_new > 0 && (int64_t)T[b] + max_new > S_)
        throw Error("generate_batch(): prompt + max_new exceeds max_seq (sequence " +
                    std::to_string(b) + ": " + std::to_string(T[b]) + " + " +
                    std::to_string(max_new) + " > " + std::to_string(S_) + ")");
      for (int i = offsets[b]; i < offsets[b + 1]; ++i)
        if (tokens[i] < 0 || tokens[i] >= c.V)
          throw Error("generate_batch(): token id " + std::to_string(tokens[i]) +
                      " is outside [0, " + std::to_string(c.V) + ")");
    }
    for (int b = 0; b < B; ++b) out_len[b] = 0;
    if (max_new <= 0) return;
    batch_alloc(B);
    Mode mode = mode_of(smp);
    mode.fused = false;
    struct Restore {  // the generation's own cache and launch choice, whatever happens
      Llama* s;
      ~Restore() {
        s->cur_ = s->kv_.at(0);
        s->short_step_ = false;
      }
    } restore{this};
    const size_t V = c.V;
    const auto t0 = std::chrono::steady_clock::now();
    // ---- prefill: distinct prompts once each; src[b] = the first sequence with b's prompt
    std::vector<int> src(B);
    for (int b = 0; b < B; ++b) {
      src[b] = b;
      for (int a = 0; a < b && src[b] == b; ++a)
        if (src[a] == a && T[a] == T[b] &&
            std::equal(tokens + offsets[a], tokens + offsets[a + 1], tokens + offsets[b]))
          src[b] = a;
    }
    std::vector<int32_t> h_len(B), h_pos(B);
    for (int b = 0; b < B; ++b) {
      h_len[b] = T[b];
      h_pos[b] = T[b] - 1;
      hip_check(hipMemcpyAsync(b_.hist + (size_t)b * S_, tokens + offsets[b], sizeof(int32_t) * T[b],
                               hipMemcpyHostToDevice, st_), "hist H2D");
    }
    hip_check(hipMemcpyAsync(b_.hist_len, h_len.data(), sizeof(int32_t) * B, hipMemcpyHostToDevice,
                             st_), "hist_len H2D");
    hip_check(hipMemcpyAsync(b_.pos, h_pos.data(), sizeof(int32_t) * B, hipMemcpyHostToDevice, st_),
              "pos H2D");
    hip_check(hipMemsetAsync(b_.slot, 0, sizeof(unsigned long long) * kMaxBatch, st_), "slot");
    hip_check(hipStreamSynchronize(st_), "sync");  // h_len / h_pos are read by the copies
    const size_t row_bytes = (size_t)lc_.hd * kv_esize();
    for (int b = 0; b < B; ++b) {
      if (src[b] != b) continue;
      cur_ = b_.kv[b];
      prefill_body(tokens + offsets[b], T[b]);
      head_gemv(hidden_ + (size_t)(T[b] - 1) * c.H);
      for (int d = b; d < B; ++d) {
        if (src[d] != b) continue;
        hip_check(hipMemcpyAsync(b_.logits + (size_t)d * V, logits_, sizeof(float) * V,
                                 hipMemcpyDeviceToDevice, st_), "logits D2D");
        if (d == b) continue;
        // rows [0, T) of every (layer, kv head) of the prefilled caches
        const size_t pitch = (size_t)S_ * row_bytes, width = (size_t)T[b] * row_bytes;
        const size_t height = owned_.size() * (size_t)lc_.nkv;
        hip_check(hipMemcpy2DAsync(b_.kv[d].k, pitch, b_.kv[b].k, pitch, width, height,
                                   hipMemcpyDeviceToDevice, st_), "k prefix D2D");
        hip_check(hipMemcpy2DAsync(b_.kv[d].v, pitch, b_.kv[b].v, pitch, width, height,
                                   hipMemcpyDeviceToDevice, st_), "v prefix D2D");
      }
    }
    // ---- first tokens, from the prefill logits
    auto mode_of_seq = [&](int b) {
      Mode m = mode;
      if (!m.greedy) m.seed = smp.seed + (uint64_t)b;
      return m;
    };
    auto select_all = [&]() {
      for (int b = 0; b < B; ++b)
        select_tail(mode_of_seq(b), {b_.logits + (size_t)b * V, b_.hist + (size_t)b * S_,
                                     b_.hist_len + b, b_.tok + b, b_.pos + b, b_.slot + b});
    };
    auto keep_logits = [&](int i) {  // token index i of every sequence
      if (!logits_out) return;
      for (int b = 0; b < B; ++b)
        hip_check(hipMemcpyAsync(logits_out + ((size_t)b * max_new + i) * V,
                                 b_.logits + (size_t)b * V, sizeof(float) * V,
                                 hipMemcpyDeviceToHost, st_), "logits D2H");
    };
    select_all();
    keep_logits(0);
    hip_check(hipMemcpyAsync(b_.host_tok, b_.tok, sizeof(int32_t) * B, hipMemcpyDeviceToHost, st_),
              "tok D2H");
    hip_check(hipStreamSynchronize(st_), "sync");
    const auto t1 = std::chrono::steady_clock::now();
    std::vector<char> done(B, 0);
    int live = B;
    auto take = [&](int i, const int32_t* toks) {  // token index i as read back
      for (int b = 0; b < B; ++b) {
        if (done[b]) continue;
        out[(size_t)b * max_new + i] = toks[b];
        out_len[b] = i + 1;
        for (int e = 0; e < n_eos; ++e)
          if (eos[e] == toks[b]) done[b] = 1;
        if (done[b]) --live;
      }
    };
    take(0, b_.host_tok);
    // ---- steps: token index i comes from step i; the host reads step i - 1 while step i runs
    std::vector<hipEvent_t> ev;
    struct Events {
      std::vector<hipEvent_t>& v;
      ~Events() { for (hipEvent_t e : v) (void)hipEventDestroy(e); }
    } events{ev};
    auto mark = [&]() {
      hipEvent_t e;
      hip_check(hipEventCreate(&e), "hipEventCreate");
      ev.push_back(e);
      hip_check(hipEventRecord(e, st_), "hipEventRecord");
    };
    mark();
    int launched = 0, taken = 0;  // steps
    auto take_step = [&](int i) {
      hip_check(hipEventSynchronize(ev[i]), "hipEventSynchronize");
      take(i, b_.host_tok + (i & 1) * kMaxBatch);
      taken = i;
    };
    for (int i = 1; i < max_new && live > 0; ++i) {
      batch_step(B, T, i);
      select_all();
      keep_logits(i);
      hip_check(hipMemcpyAsync(b_.host_tok + (i & 1) * kMaxBatch, b_.tok, sizeof(int32_t) * B,
                               hipMemcpyDeviceToHost, st_), "tok D2H");
      mark();
      launched = i;
      if (i >= 2) take_step(i - 1);
    }
    if (launched > taken && live > 0) take_step(launched);
    hip_check(hipStreamSynchronize(st_), "sync");
    const auto t2 = std::chrono::steady_clock::now();
    check_attn_error("generate_batch");
    std::vector<float> ms;
    for (int i = 1; i <= launched; ++i) {
      float t = 0.f;
      hip_check(hipEventElapsedTime(&t, ev[i - 1], ev[i]), "hipEventElapsedTime");
      ms.push_back(t);
    }
    const double prefill_s = std::chrono::duration<double>(t1 - t0).count();
    const double decode_s = std::chrono::duration<double>(t2 - t1).count();
    int n_prompt = 0, n_gen = 0, n_steps = 0;
    for (int b = 0; b < B; ++b) {
      if (seq_stats) fill_stats(seq_stats + b, T[b], out_len[b], prefill_s, decode_s, ms);
      n_prompt += T[b];
      n_gen += out_len[b];
      n_steps += out_len[b] - 1;
    }
    if (stats) {
      fill_stats(stats, n_prompt, n_gen, prefill_s, decode_s, ms);
      stats->tokens_per_s = decode_s > 0 ? n_steps / decode_s : 0.0;  // all sequences together
    }
  }

  // A tensor-parallel rank's callback never stops the generation (every rank must replay
  // the same steps: they all stop at the same EOS token, which each reads back itself);
  // the lead's callback only sees the tokens.
  struct TpStop {
    cake_engine_token_cb cb;
    void* ctx;
    bool stopped;
  };
  static int32_t tp_token_cb(void* vctx, int32_t tok) {
    auto* t = static_cast<TpStop*>(vctx);
    if (!t->stopped && t->cb && t->cb(t->ctx, tok) != 0) t->stopped = true;
    return 0;
  }

  // counts a token's record as readable (cake_engine_logprobs) before the caller sees it
  struct LpCb {
    Llama* self;
    cake_engine_token_cb cb;
    void* ctx;
  };
  static int32_t lp_token_cb(void* vctx, int32_t tok) {
    auto* c = static_cast<LpCb*>(vctx);
    ++c->self->lp_n_;
    return c->cb ? c->cb(c->ctx, tok) : 0;
  }
  // host copy of this call's records: room for max_new of them, none yet
  void lp_begin(bool on, int max_new) {
    lp_on_ = on;
    lp_n_ = 0;
    if (lp_on_) lp_host_.assign((size_t)max_new * kLpRecWords, 0u);
  }

  static Json eos_json(const int32_t* eos, int n_eos) {
    Json a = Json::array();
    for (int i = 0; i < n_eos; ++i) a.push(Json::integer(eos[i]));
    return a;
  }

  // n tokens of graph replays after history length L (device position L - 1); 0 or the
  // tokens kept (lead: written to out, EOS inclusive); per-token device ms in *ms_out
  int decode_tokens(int L, int n, const int32_t* eos, int n_eos, cake_engine_token_cb cb,
                    void* ctx, int32_t* out, int out_cap, bool lead, std::vector<float>* ms_out) {
    std::vector<int32_t> toks(n);
    std::vector<float> ms(n, 0.f);
    CakeLoopSpec spec{};
    std::vector<void*> execs(execs_.begin(), execs_.end());
    spec.execs = execs.data();
    spec.n_execs = (int32_t)execs.size();
    spec.bucket_of = bucket_of_.data();
    spec.n_len = (int32_t)bucket_of_.size();
    spec.k = k_;
    spec.hist = hist_;
    spec.base = L;      // history index of the first token of this run
    spec.pos = L - 1;   // device position (last written row)
    spec.n = n;
    spec.chunk = 0;
    AnnounceCtx actx{this, L - 1};
    if (world_ > 1) {  // the workers enqueue each chunk of replays when told
      spec.chunk = kAnnounceChunk;
      spec.announce = &Llama::announce_cb;
      spec.announce_ctx = &actx;
    }
    spec.eos = eos;
    spec.n_eos = n_eos;
    spec.on_token = cb;
    spec.token_ctx = ctx;
    spec.stream = st_;
    spec.out_tokens = toks.data();
    spec.out_ms = ms.data();
    spec.out_cap = n;
    LpCb lpc{this, cb, ctx};
    if (lp_on_ && lead) {  // the records ride the read-back ring with their tokens
      spec.rec = lp_rec_;
      spec.rec_bytes = kLpRecWords * 4;
      spec.out_rec = lp_host_.data() + (size_t)lp_n_ * kLpRecWords;
      spec.on_token = &Llama::lp_token_cb;
      spec.token_ctx = &lpc;
    }
    TpStop tps{cb, ctx, false};
    if (tp_ > 1) {  // lock step: every rank reads the tokens back and stops at EOS
      spec.on_token = lead ? &Llama::tp_token_cb : nullptr;
      spec.token_ctx = &tps;
    }
    CakeLoopResult res{};
    trace(rank(), "decode " + std::to_string(n) + " tokens from length " + std::to_string(L));
    const int rc = cake_graph_decode(&spec, &res);
    trace(rank(), "decode loop done: " + std::to_string(res.n_tokens) + " tokens, " +
                      std::to_string(res.replays) + " replays, rc " + std::to_string(rc));
    if (world_ > 1) sync_workers(hop_drain());
    if (tp_ > 1 && lead) sync_workers(ar_drain());
    k_check(rc, "graph_decode");
    if (lead) check_attn_error("rank " + std::to_string(rank()));  // TP workers: in "sync"
    int n_out = 0;
    if (lead)
      for (int i = 0; i < res.n_tokens && n_out < out_cap; ++i) out[n_out++] = toks[i];
    ms.resize(lead ? res.n_tokens : 0);
    if (ms_out) *ms_out = std::move(ms);
    return n_out;
  }

  void fill_stats(CakeEngineStats* stats, int n_prompt, int n_out, double prefill_s,
                  double decode_s, const std::vector<float>& ms) const {
    stats->n_prompt = n_prompt;
    stats->n_generated = n_out;
    stats->prefill_s = prefill_s;
    stats->decode_s = decode_s;
    stats->tokens_per_s = n_out > 1 && decode_s > 0 ? (n_out - 1) / decode_s : 0.0;
    std::vector<float> s = ms;
    std::sort(s.begin(), s.end());
    auto pct = [&](double q) {
      if (s.empty()) return 0.f;
      const size_t i = std::min(s.size() - 1, (size_t)std::llround(q / 100.0 * (s.size() - 1)));
      return s[i];
    };
    stats->p50_ms = pct(50);
    stats->p99_ms = pct(99);
  }

  void run_generation(const int32_t* prompt, int T, int max_new, const CakeEngineSampling& smp,
                      const int32_t* eos, int n_eos, cake_engine_token_cb cb, void* ctx,
                      int32_t* out, int out_cap, CakeEngineStats* stats, bool lead) {
    const auto t0 = std::chrono::steady_clock::now();
    prefill_body(prompt, T);
    // the prefill position bookkeeping of DeviceDecoder.start: history = prompt,
    // pos = T - 1 (the last written row), slot cleared
    std::vector<int32_t> h(prompt, prompt + T);
    hip_check(hipMemcpyAsync(hist_, h.data(), sizeof(int32_t) * T, hipMemcpyHostToDevice, st_),
              "hist H2D");
    set_i32(hist_len_, T);
    set_i32(pos_, T - 1);
    hip_check(hipMemsetAsync(slot_, 0, sizeof(unsigned long long), st_), "slot");
    Mode mode = mode_of(smp);
    if (mode.controls) lc_begin(T, mode);
    // first token from the prefill logits (DeviceDecoder._select_first)
    if (tp_ > 1) {
      head_tp(hidden_ + (size_t)(T - 1) * cfg_.H, mode);
    } else {
      head_gemv(hidden_ + (size_t)(T - 1) * cfg_.H);
      select_tail(mode);
      logprob_record(mode);
    }
    if (mode.fused) k_check(cake_embed(dt_, embed_, tok_, 1, cfg_.H, resid_, st_), "embed");
    int32_t first = 0;
    hip_check(hipMemcpyAsync(&first, tok_, sizeof(int32_t), hipMemcpyDeviceToHost, st_), "tok");
    lp_begin(mode.logprobs >= 0, max_new);
    if (lp_on_)  // the first token sits at history index T
      hip_check(hipMemcpyAsync(lp_host_.data(), lp_rec_ + (size_t)T * kLpRecWords,
                               kLpRecWords * 4, hipMemcpyDeviceToHost, st_), "logprob D2H");
    hip_check(hipStreamSynchronize(st_), "sync");
    if (lp_on_ && lead) lp_n_ = 1;
    const auto t1 = std::chrono::steady_clock::now();
    int n_out = 0;
    bool stop = false;
    for (int e = 0; e < n_eos && !stop; ++e)
      if (eos[e] == first) stop = true;
    if (lead) {
      out[n_out++] = first;
      const bool cb_stop = cb && cb(ctx, first) != 0;
      if (tp_ == 1) stop = stop || cb_stop;  // TP: only EOS stops (all ranks alike)
    }
    std::vector<float> ms;
    last_mode_ = mode;
    if (remote_mode()) {  // host round trips inside the step: eager
      have_graphs_ = true;  // continue() may follow
      if (!stop && max_new > 1)
        n_out += decode_eager(T, max_new - 1, mode, eos, n_eos, cb, ctx, out + n_out,
                              out_cap - n_out, &ms);
    } else {
      // graphs exist after every generation (continue() replays them), even a 1-token one
      ensure_graphs(mode);
      if (!stop && max_new > 1)
        n_out += decode_tokens(T + 1, max_new - 1, eos, n_eos, cb, ctx,
                               lead ? out + n_out : nullptr, lead ? out_cap - n_out : 0, lead, &ms);
    }
    const auto t2 = std::chrono::steady_clock::now();
    if (stats)
      fill_stats(stats, T, n_out, std::chrono::duration<double>(t1 - t0).count(),
                 std::chrono::duration<double>(t2 - t1).count(), ms);
  }

  int read_i32(const int* p) {
    int v = 0;
    hip_check(hipMemcpyAsync(&v, p, sizeof(int), hipMemcpyDeviceToHost, st_), "i32 D2H");
    hip_check(hipStreamSynchronize(st_), "sync");
    return v;
  }

  // the split-K attention merge's error word (tickets[2 nkv], attn_core2.h): a merge
  // that gave up waiting for its partials left that launch's outputs invalid
  void check_attn_error(const std::string& who) {
    unsigned int w = 0;
    hip_check(hipMemcpyAsync(&w, tickets_ + 2 * lc_.nkv, sizeof(w), hipMemcpyDeviceToHost, st_),
              "attn err D2H");
    hip_check(hipStreamSynchronize(st_), "sync");
    if (w) {
      hip_check(hipMemsetAsync(tickets_ + 2 * lc_.nkv, 0, sizeof(unsigned int), st_), "attn err");
      hip_check(hipStreamSynchronize(st_), "sync");
      throw Error(who + ": decode attention split merge timed out waiting for its partials; "
                        "the tokens of that generation are invalid");
    }
  }

 private:
  // One layer: the two norm vectors and its four projections, each a Mat (llama_weights.h) in
  // the engine's weight_fmt: q | k | v rows and gate | up rows are one matrix each, and the
  // GEMV dispatchers take the row blocks out of it.
  struct LayerW {
    void *ln1 = nullptr, *ln2 = nullptr;
    Mat qkv, o, gu, d;
  };
  // CAKE_PACK16 (docs/ENV.md): the lossless 13-bit copies of the bf16 projections and lm_head
  // (kernels/gemv_p13_kernel.h; Mat::p13) the decode GEMVs stream instead of the 16-bit rows,
  // which stay resident for prefill, the f16 path, tensor parallelism and the oracles
  int64_t packed_bytes_ = 0;
  int packed_mats_ = 0, packed_raw_rows_ = 0;
  bool pack_full_ = false;  // the HBM reserve was reached: the matrices after it stay 16-bit
  struct Mode {
    bool fused = true;  // greedy with the fused head_select tail
    bool greedy = true;
    float temperature = 0.f, top_p = 0.f, penalty = 1.f;
    int top_k = 0, last_n = 0;
    unsigned long long seed = 0;
    int logprobs = -1;  // >= 0: a log-prob record per token with that many alternatives
    // logit controls: only on / off is part of the graphs; the values live in lc_params_
    bool controls = false;  // the cake_logit_controls launch runs in select_tail
    bool min_p = false;     // sampled, min_p on: its cut key joins the draw's threshold
    bool operator==(const Mode& o) const {
      return std::tie(fused, greedy, temperature, top_p, penalty, top_k, last_n, seed,
                      logprobs, controls, min_p) ==
             std::tie(o.fused, o.greedy, o.temperature, o.top_p, o.penalty, o.top_k, o.last_n,
                      o.seed, o.logprobs, o.controls, o.min_p);
    }
  };
  // cake_engine_set_logit_controls, checked; on: some value is not neutral
  struct LcSetting {
    bool on = false;
    float presence = 0.f, frequency = 0.f, min_p = 0.f;
    std::vector<int32_t> ids;
    std::vector<float> vals;
  };

  int dt_, dev_, init_ = 0;
  int wfmt_ = 0;               // CakeEngineOpts.weight_fmt
  int hfmt_ = 0;               // CakeEngineOpts.head_fmt (0 on a rank without the head)
  // CakeEngineOpts.kv_fmt.  1: the session caches hold one e4m3fn byte per element; decode
  // attention is cake_attn_decode_kv8, prefill attention reads the live prefix widened into
  // kv16_k_ / kv16_v_ (one layer's [nkv][S][hd], allocated once).  2: the 16-bit cache with
  // fp8-valued writers (test oracle).  != 0: never the head-parallel or fused launches.
  int kvfmt_ = 0;
  // prefill_fmt (bits 8 and up of CakeEngineOpts.weight_fmt).  1: every prefill projection quantises its activation rows
  // (a8_ codes, sa_ one f32 scale per token) and runs cake_gemm_w8a8 on the resident codes
  int pfmt_ = 0;
  uint16_t *kv16_k_ = nullptr, *kv16_v_ = nullptr;
  int64_t weight_bytes_ = 0;   // device weight allocations of this rank
  // weight_fmt 1, 2: 16-bit scratch for the largest projection — the loader fills it before
  // each quantise (the 16-bit copy is never kept), prefill dequantises into it before
  // each GEMM
  uint16_t* w16_ = nullptr;
  bool forced_ = false;  // teacher-forcing steps: the head writes full logits
  // fused decode attention + o_proj (attn_oproj.hip) for one-split live lengths: the
  // short-context graph bucket and eager steps at such a position
  // fused attention + o_proj (csrc/experimental/attn_oproj.hip, CAKE_BUILD_EXPERIMENTAL=1;
  // measured slower than the pair: profiles/r5_attn_oproj_ab.md), looked up at run time
  AoFns ao_;
  bool ao_ok_ = false, short_step_ = false;
  int heads_max_ = 0;  // live lengths <= this: head-parallel attention (attn_head_kernel)
  float* ao_ws_ = nullptr;
  unsigned int* ao_tickets_ = nullptr;
  uint64_t seed_ = 0;
  int rank_ = 0, world_ = 1, lo_ = 0, hi_ = 0;
  bool head_ = true, hop_bf16_ = false;
  double hop_timeout_ = 30.0;
  // The token's walk (llama.rs:81-117): embedding on rank 0, then every maximal run of
  // consecutive layers on one rank, then the head on rank 0.  An edge joins consecutive
  // stops on different ranks; each edge has its own inbox on the receiving rank and its
  // own sequence words (seq_[2e] send side, seq_[2e + 1] receive side).
  enum StopKind { kEmbedStop, kRunStop, kHeadStop, kRemoteStop };
  struct Stop {
    StopKind kind;
    int rank;
    std::vector<int> layers;  // global ids (runs)
    std::vector<int> sel;     // the same as this rank's local layer slots
    int remote = -1;          // kRemoteStop: index into remotes_
  };
  // TCP workers (master side): one connection each, Hello -> WorkerInfo at open
  struct RemoteWorker {
    std::string addr;
    int fd;
  };
  std::vector<RemoteWorker> remotes_;
  std::vector<int> remote_of_;  // layer -> remote worker, -1 = local
  double remote_timeout_ = 60.0;
  std::vector<float> host_rows_;  // staging of the hidden rows a remote run transforms
  std::vector<Stop> walk_;
  std::vector<int> edge_in_;                // per stop: the edge feeding it, or -1
  std::vector<std::pair<int, int>> edges_;  // (src rank, dst rank)
  std::vector<int> owner_;                  // layer -> pipeline rank
  std::map<int, void*> my_inbox_;           // edge -> own inbox (edges into this rank)
  std::map<int, void*> out_inbox_;          // edge -> IPC-mapped inbox of the receiver
  std::map<int, void*> peer_pbuf_;          // rank -> IPC-mapped prefill relay buffer
  // prefill rows a peer hands to this rank land here (uncached device memory, IPC-exported,
  // written over xGMI by the sender's copy), then one local copy moves them into hidden_:
  // hidden_ itself stays ordinary cached memory for the GEMM epilogues, and no L2 line of
  // this device can hold a stale copy of what the peer wrote
  float* relay_ = nullptr;
  unsigned int* seq_ = nullptr;
  int* hop_err_ = nullptr;
  Star ctl_;  // control sockets of the pipeline or tensor-parallel ranks, rank 0 the hub
  // tensor parallel
  struct ArChan {
    void* inbox = nullptr;
    std::vector<void*> peers;  // peer inboxes (IPC-mapped), own slot unused
  };

  int tp_ = 1, tp_rank_ = 0, i0_ = 0, voff_ = 0, slab_bank_ = 0;
  // rows of one prefill all-reduce round: the slab (2 banks x tp slots x rows x H f32,
  // uncached, IPC-mapped by every peer) is sized for this many rows, a longer prefill
  // runs in rounds — a slab sized for max_seq (2 GB per rank at 70B tp8, 4096 keys) made
  // the eight peer imports stall on one shared GPU
  static constexpr int kSlabRows = 512;
  Cfg lc_;                   // this rank's compute shapes (the whole model unless TP)
  ArChan ch_sum_, ch_key_, ch_gat_;
  float *partial_ = nullptr, *ppart_ = nullptr, *full_logits_ = nullptr, *slab_ = nullptr;
  unsigned int* ar_seq_ = nullptr;
  int* ar_err_ = nullptr;
  std::vector<void*> peer_slab_, tp_mapped_, tp_owned_;
  hipStream_t st_ = nullptr;
  Cfg cfg_;
  int S_ = 0, k_ = 1;
  GemmPlanner planner_;
  std::vector<void*> allocs_;
  void *embed_ = nullptr, *norm_ = nullptr;
  // the lm_head [V, H] in head_fmt (this rank's vocabulary rows under tensor parallelism).
  // 16-bit with tied embeddings: embed_ itself; quantised: its own codes, tied or not, and
  // embed_ stays for the gather.  Empty on a rank without the head.
  Mat lm_head_;
  std::vector<LayerW> layers_;
  struct KV { uint8_t *k, *v; };            // [local layers][nkv][S][hd], kv_esize() bytes each
  std::map<uint64_t, KV> kv_;
  std::list<uint64_t> lru_;
  KV cur_{nullptr, nullptr};
  std::vector<int> owned_, local_;          // global layer ids served here / inverse map
  float* inv_freq_ = nullptr;
  // decode state (graph-stable addresses; DecodeBuffers)
  float *resid_ = nullptr, *q_ = nullptr, *part_ = nullptr, *logits_ = nullptr;
  void *attn_out_ = nullptr, *act_ = nullptr;
  unsigned int *tickets_ = nullptr, *thr_ = nullptr, *sel_ticket_ = nullptr;
  int *pos_ = nullptr, *tok_ = nullptr, *hist_ = nullptr, *hist_len_ = nullptr;
  unsigned long long* slot_ = nullptr;
  int* scratch_i32_ = nullptr;  // warm-up snapshot: tok, pos, hist_len
  float* scratch_resid_ = nullptr;
  int32_t* zeros_ = nullptr;    // 64 zero words (GEMM LDS-DMA padding source)
  // prefill buffers (grown to the longest prompt)
  int pre_T_ = 0;
  float* hidden_ = nullptr;
  void *x16_ = nullptr, *qkv_ = nullptr, *att_ = nullptr, *pact_ = nullptr;
  int32_t* ptok_ = nullptr;
  uint8_t* a8_ = nullptr;       // prefill_fmt 1: [T, max(H, nq, I)] activation codes
  float* sa_ = nullptr;         // prefill_fmt 1: [T] activation scales
  // scoring scratch (first score() call; grown like the prefill buffers): the f32 logit
  // chunk [rows, Vc], the 16-bit copy of a quantised head's chunk [Vc, H], per-row state
  int sc_T_ = 0, sc_Vc_ = 0;
  float *sc_logits_ = nullptr, *sc_max_ = nullptr, *sc_tgt_ = nullptr, *sc_lse_ = nullptr,
        *sc_topv_ = nullptr;
  double* sc_sum_ = nullptr;
  unsigned long long* sc_key_ = nullptr;
  int32_t *sc_target_ = nullptr, *sc_top_ = nullptr;
  uint16_t* sc_head_ = nullptr;
  // log-probs of generated tokens (set_logprobs): device records indexed like hist_, the
  // kernel's partials and ticket; the host copy holds the last call's records in token order
  int lp_k_ = -1;       // the next generate()'s setting
  bool lp_on_ = false;  // the last generate() / continue() call recorded
  int lp_n_ = 0;        // its records readable so far
  uint32_t* lp_rec_ = nullptr;
  uint8_t* lp_ws_ = nullptr;
  unsigned int* lp_ticket_ = nullptr;
  std::vector<uint32_t> lp_host_;
  // logit controls (set_logit_controls): the next generate()'s setting, the count table [V],
  // the parameter block and the state words of kernels/logit_controls.hip
  LcSetting lc_next_;
  unsigned int *lc_cnt_ = nullptr, *lc_params_ = nullptr, *lc_state_ = nullptr;
  std::vector<uint32_t> lc_host_;  // the block of the running generation (H2D source)
  float* ws_ = nullptr;
  size_t ws_n_ = 0;
  static constexpr size_t kLibWsBytes = 32u << 20;
  uint8_t* lib_ws_ = nullptr;   // hipBLASLt workspace (first library GEMM)
  uint16_t* pgu_ = nullptr;     // [T, 2I] gate|up product of a library SwiGLU GEMM
  size_t pgu_n_ = 0;
  // decode graphs
  std::vector<hipGraphExec_t> execs_;
  std::vector<hipGraph_t> graphs_;
  std::vector<int32_t> bucket_of_;
  Mode graph_mode_, last_mode_;
  bool have_graphs_ = false;
  // lock-step batched decode (generate_batch): nothing of it exists before the first call
  static constexpr int kMaxBatch = 8;
  struct BatchState {
    std::vector<KV> kv;  // one K / V cache set per sequence
    float *resid = nullptr, *qkv32 = nullptr, *q = nullptr, *logits = nullptr;  // [8, ...] rows
    float* logits2 = nullptr;  // [16, V]: the head's two partial rows per sequence
    uint16_t *x16 = nullptr, *attn = nullptr, *act = nullptr;  // x16: [16, H]
    int *tok = nullptr, *pos = nullptr, *hist = nullptr, *hist_len = nullptr;  // hist: [8, S]
    unsigned long long* slot = nullptr;
    void **kbase = nullptr, **vbase = nullptr;  // device tables of the sequences' cache bases
    int32_t* host_tok = nullptr;                // pinned: two rows of 8, the read-back ring
  } b_;

  template <class T> T* dalloc(size_t n) {
    void* p = nullptr;
    hip_check(hipMalloc(&p, std::max<size_t>(n * sizeof(T), 16)), "hipMalloc");
    allocs_.push_back(p);
    return reinterpret_cast<T*>(p);
  }
  void dfree(void* p) {
    if (!p) return;
    auto it = std::find(allocs_.begin(), allocs_.end(), p);
    if (it != allocs_.end()) allocs_.erase(it);
    (void)hipFree(p);
  }

  void set_i32(int* p, int v) {
    hip_check(hipMemcpyAsync(p, &v, sizeof(int), hipMemcpyHostToDevice, st_), "i32 H2D");
    hip_check(hipStreamSynchronize(st_), "sync");  // &v is a stack value
  }

  // ---- weights
  void upload(Checkpoint& ck, const std::string& name, void* dst, size_t numel, void*& stage,
              size_t& stage_bytes) {
    const TensorView& t = ck.tensor(name);
    size_t n = 1;
    for (auto d : t.shape) n *= d;
    if (n != numel) throw Error(name + ": " + std::to_string(n) + " elements, expected " +
                                std::to_string(numel));
    const size_t R = t.shape.empty() ? 1 : t.shape[0];
    upload_slice(ck, name, dst, 0, R, 0, n / R, stage, stage_bytes);
  }

  // rows [r0, r0 + nr) x columns [c0, c0 + nc) of a 2-D tensor (1-D: one column) into
  // dst as a dense [nr, nc] block in the model dtype (column slices gathered on the host)
  void upload_slice(Checkpoint& ck, const std::string& name, void* dst, size_t r0, size_t nr,
                    size_t c0, size_t nc, void*& stage, size_t& stage_bytes) {
    const TensorView& t = ck.tensor(name);
    int kind;
    if (t.dtype == "BF16") kind = 0;
    else if (t.dtype == "F16") kind = 1;
    else if (t.dtype == "F32") kind = 2;
    else throw Error(name + ": unsupported dtype " + t.dtype);
    const size_t es = kind == 2 ? 4 : 2;
    const size_t R = t.shape.empty() ? 1 : t.shape[0];
    const size_t C = R ? (t.nbytes / es) / R : 0;
    if (r0 + nr > R || c0 + nc > C) throw Error(name + ": slice outside the tensor");
    const uint8_t* src = t.data + (r0 * C + c0) * es;
    std::vector<uint8_t> tmp;
    if (nc != C) {
      tmp.resize(nr * nc * es);
      for (size_t r = 0; r < nr; ++r)
        std::memcpy(tmp.data() + r * nc * es, t.data + ((r0 + r) * C + c0) * es, nc * es);
      src = tmp.data();
    }
    const size_t bytes = nr * nc * es, n = nr * nc;
    if (kind == dt_) {
      hip_check(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice), "weight H2D");
      return;
    }
    if (stage_bytes < bytes) {
      if (stage) (void)hipFree(stage);
      hip_check(hipMalloc(&stage, bytes), "hipMalloc stage");
      stage_bytes = bytes;
    }
    hip_check(hipMemcpy(stage, src, bytes, hipMemcpyHostToDevice), "weight H2D");
    k_check(cake_cast16(kind, dt_, stage, dst, n, st_), "cast16");
    hip_check(hipStreamSynchronize(st_), "sync");
  }

  // a 16-bit weight tensor of n elements (counted in weight_bytes_)
  uint16_t* walloc16(size_t n) {
    weight_bytes_ += (int64_t)n * 2;
    return dalloc<uint16_t>(n);
  }
  // where the loader writes the 16-bit rows of an [N, K] matrix kept in format fmt: its own
  // allocation (16-bit), the shared scratch sized for the largest projection (quantised), or
  // with `temp` a buffer of its own (the [V, H] of a quantised untied head: not counted, keep()
  // frees it before open returns, so an open peaks at the resident weights + 2 V H bytes)
  uint16_t* stage(int fmt, size_t N, size_t K, bool temp = false) {
    if (fmt == kFmt16) return walloc16(N * K);
    if (temp) return dalloc<uint16_t>(N * K);
    if (!w16_) {
      const size_t H = cfg_.H, nq = (size_t)lc_.nh * cfg_.hd, nk = (size_t)lc_.nkv * cfg_.hd;
      const size_t I = lc_.I;
      w16_ = dalloc<uint16_t>(std::max({(nq + 2 * nk) * H, H * nq, 2 * I * H, H * I}));
    }
    return w16_;
  }
  // the matrix whose 16-bit rows `staged` holds: the rows as they are, or quantised into its
  // own codes + side data (llama_weights.h quantise); the scratch is free again on return.
  // `temp`: staged is stage()'s temporary and is freed (else the resident embedding)
  Mat keep(int fmt, uint16_t* staged, size_t N, size_t K, bool temp = false) {
    Mat m{fmt, N, K, staged};
    if (fmt == kFmt16) return m;
    m.w = dalloc<uint8_t>(fmt_code_bytes(fmt, N, K));
    if (fmt == kFmtFp8) m.scale = dalloc<float>(N);
    else m.e8 = dalloc<uint8_t>(fmt_side_bytes(fmt, N, K));
    weight_bytes_ += (int64_t)m.bytes();
    k_check(quantise(m, staged, dt_, st_), fmt == kFmtFp8 ? "quant_rows_fp8" : "quant_rows_mxfp4");
    hip_check(hipStreamSynchronize(st_), "sync");
    if (temp) dfree(staged);
    return m;
  }

  // weights of this rank: all of the model, its pipeline layers, or (tensor parallel) its
  // slices — q / k / v rows of its heads, o_proj columns of its heads, gate / up rows and
  // down_proj columns of its intermediate range, lm_head rows of its vocabulary range
  // (parallel/tensor_parallel.py shard_block / shard_head).  One list names a layer's tensors
  // for both loaders, so a random_init engine has a checkpoint's shapes and packing.
  struct Part { const char* name; size_t r0, nr, c0, nc; };  // a checkpoint tensor's slice
  struct LayerTensor {
    void* LayerW::*vec;  // a norm vector [N], or
    Mat LayerW::*mat;    // a projection [N, K]: the parts' rows packed in order
    size_t N, K;
    uint64_t tag;  // random init: drawn whole (not per part) with tag 16 + 16 layer + tag
    std::vector<Part> parts;
  };
  std::vector<LayerTensor> layer_tensors() const {
    const size_t H = cfg_.H, hd = cfg_.hd, nq = lc_.nh * hd, nk = lc_.nkv * hd, I = lc_.I;
    const size_t q0 = tp_rank_ * nq, k0 = tp_rank_ * nk, i0 = i0_;
    return {
        {&LayerW::ln1, nullptr, H, 1, 0, {{"input_layernorm.weight", 0, H, 0, 1}}},
        {nullptr, &LayerW::qkv, nq + 2 * nk, H, 1,
         {{"self_attn.q_proj.weight", q0, nq, 0, H},
          {"self_attn.k_proj.weight", k0, nk, 0, H},
          {"self_attn.v_proj.weight", k0, nk, 0, H}}},
        {nullptr, &LayerW::o, H, nq, 2, {{"self_attn.o_proj.weight", 0, H, q0, nq}}},
        {&LayerW::ln2, nullptr, H, 1, 3, {{"post_attention_layernorm.weight", 0, H, 0, 1}}},
        {nullptr, &LayerW::gu, 2 * I, H, 4,
         {{"mlp.gate_proj.weight", i0, I, 0, H}, {"mlp.up_proj.weight", i0, I, 0, H}}},
        {nullptr, &LayerW::d, H, I, 5, {{"mlp.down_proj.weight", 0, H, i0, I}}},
    };
  }
  // every owned layer's tensors: allocated (norms) or staged and kept (projections), their
  // 16-bit values written by fill(layer, tensor, dst)
  void load_layers(const std::function<void(int, const LayerTensor&, uint16_t*)>& fill) {
    const std::vector<LayerTensor> tensors = layer_tensors();
    layers_.resize(owned_.size());
    for (int l : owned_) {
      LayerW& w = layers_[local_[l]];
      for (const LayerTensor& t : tensors) {
        uint16_t* p = t.vec ? walloc16(t.N) : stage(wfmt_, t.N, t.K);
        fill(l, t, p);
        if (t.vec) w.*t.vec = p;
        else w.*t.mat = keep(wfmt_, p, t.N, t.K);
      }
    }
  }
  // the lm_head of this rank's vocabulary rows: the embedding's rows when tied, else its own,
  // written by fill(dst)
  void load_head(bool tied, const std::function<void(uint16_t*)>& fill) {
    const size_t V = lc_.V, H = cfg_.H;
    uint16_t* p = tied ? static_cast<uint16_t*>(embed_) : stage(hfmt_, V, H, true);
    if (!tied) fill(p);
    lm_head_ = keep(hfmt_, p, V, H, !tied);
  }

  // init = 1: this rank's tensors (same shapes and packing as a checkpoint load) drawn
  // on the device — N(0, 0.02) linears and lm_head, N(0, 1) embedding, N(1, 0.05) norms
  // (models/llama3/weights.py random) — keyed by (seed, layer, tensor)
  void load_random() {
    const size_t H = cfg_.H, V = cfg_.V;
    auto fill = [&](void* p, size_t n, float mean, float std, uint64_t tag) {
      const uint64_t key = seed_ * 0x9e3779b97f4a7c15ULL + tag * 0xc2b2ae3d27d4eb4fULL +
                           (uint64_t)tp_rank_ * 0x165667b19e3779f9ULL;
      k_check(cake_fill_normal(dt_, p, n, mean, std, key, st_), "fill_normal");
    };
    if (head_) {
      embed_ = walloc16(V * H);
      fill(embed_, V * H, 0.f, 1.f, 1);
      norm_ = walloc16(H);
      fill(norm_, H, 1.f, 0.05f, 2);
      load_head(cfg_.tie && tp_ == 1,  // (the same draws whatever the head format)
                [&](uint16_t* hw) { fill(hw, (size_t)lc_.V * H, 0.f, 0.02f, 3); });
    }
    load_layers([&](int l, const LayerTensor& t, uint16_t* dst) {
      fill(dst, t.N * t.K, t.vec ? 1.f : 0.f, t.vec ? 0.05f : 0.02f, 16 + 16 * (uint64_t)l + t.tag);
    });
    hip_check(hipStreamSynchronize(st_), "sync");
  }

  void load_weights(const std::string& dir) {
    if (init_ == 1) {
      load_random();
      return;
    }
    Checkpoint ck(dir);
    const size_t H = cfg_.H, V = cfg_.V;
    void* stage = nullptr;
    size_t stage_bytes = 0;
    try {
      if (head_) {
        embed_ = walloc16(V * H);
        upload(ck, "model.embed_tokens.weight", embed_, V * H, stage, stage_bytes);
        norm_ = walloc16(H);
        upload(ck, "model.norm.weight", norm_, H, stage, stage_bytes);
        const bool own_head = ck.has("lm_head.weight") && !cfg_.tie;
        const char* hn = own_head ? "lm_head.weight" : "model.embed_tokens.weight";
        load_head(tp_ == 1 && !own_head, [&](uint16_t* hw) {
          if (tp_ > 1) upload_slice(ck, hn, hw, voff_, lc_.V, 0, H, stage, stage_bytes);
          else upload(ck, hn, hw, V * H, stage, stage_bytes);
        });
      }
      load_layers([&](int l, const LayerTensor& t, uint16_t* dst) {
        const std::string p = "model.layers." + std::to_string(l) + ".";
        if (t.vec) return upload(ck, p + t.parts[0].name, dst, t.N, stage, stage_bytes);
        for (const Part& s : t.parts) {
          upload_slice(ck, p + s.name, dst, s.r0, s.nr, s.c0, s.nc, stage, stage_bytes);
          dst += s.nr * t.K;
        }
      });
    } catch (...) {
      if (stage) (void)hipFree(stage);
      throw;
    }
    if (stage) (void)hipFree(stage);
  }


  void alloc_state() {
    const Cfg& c = lc_;
    kv_session(0);  // session 0: generation / pipeline
    if (kvfmt_ == kKvFp8) {  // prefill's 16-bit view of one layer's live prefix
      const size_t n = (size_t)c.nkv * S_ * c.hd;
      kv16_k_ = dalloc<uint16_t>(n);
      kv16_v_ = dalloc<uint16_t>(n);
      hip_check(hipMemset(kv16_k_, 0, n * 2), "memset");
      hip_check(hipMemset(kv16_v_, 0, n * 2), "memset");
    }
    const std::vector<float> f = c.inv_freq();
    inv_freq_ = dalloc<float>(f.size());
    hip_check(hipMemcpy(inv_freq_, f.data(), f.size() * sizeof(float), hipMemcpyHostToDevice),
              "inv_freq");
    const size_t nq = (size_t)c.nh * c.hd;
    // [H f32 | pos | pad]: a pipeline hop carries the position as its header word
    resid_ = dalloc<float>(c.H + 4);
    hidden_ = dalloc<float>((size_t)S_ * c.H);  // prefill hidden (peer-written in a pipeline)
    q_ = dalloc<float>(nq);
    part_ = dalloc<float>(2 * (size_t)c.nh * kMaxSplit * (c.hd + 2));
    logits_ = dalloc<float>(c.V);
    attn_out_ = dalloc<uint16_t>(nq);
    act_ = dalloc<uint16_t>(c.I);
    tickets_ = dalloc<unsigned int>(2 * c.nkv + 2);
    thr_ = dalloc<unsigned int>(1);
    sel_ticket_ = dalloc<unsigned int>(1);
    pos_ = reinterpret_cast<int*>(resid_ + c.H);
    tok_ = dalloc<int>(1);
    hist_ = dalloc<int>(S_);
    hist_len_ = dalloc<int>(1);
    slot_ = dalloc<unsigned long long>(1);
    scratch_i32_ = dalloc<int>(4);
    scratch_resid_ = dalloc<float>(c.H + 4);  // + the hop header (self-tests)
    zeros_ = dalloc<int32_t>(64);
    hip_check(hipMemset(tickets_, 0, sizeof(unsigned int) * (2 * c.nkv + 2)), "memset");
    hip_check(hipMemset(part_, 0, sizeof(float) * 2 * c.nh * kMaxSplit * (c.hd + 2)), "memset");
    hip_check(hipMemset(sel_ticket_, 0, sizeof(unsigned int)), "memset");
    hip_check(hipMemset(slot_, 0, sizeof(unsigned long long)), "memset");
    hip_check(hipMemset(zeros_, 0, sizeof(int32_t) * 64), "memset");
    hip_check(hipMemset(hist_, 0, sizeof(int) * S_), "memset");
    hip_check(hipMemset(resid_, 0, sizeof(float) * (c.H + 4)), "memset");
    // opt-in (CAKE_ATTN_OPROJ=1): measured slower than the attention + o_proj pair on
    // MI355X (profiles/r5_attn_oproj_ab.md), kept for the A/B
    {
      const char* e = std::getenv("CAKE_ATTN_OPROJ");
      // (reads o_proj as 16-bit rows: off with fp8 and mxfp4 weights)
      if (e && std::string(e) == "1" && wfmt_ == kFmt16 && kvfmt_ == kKv16) ao_ = ao_fns();
      ao_ok_ = ao_.run != nullptr && ao_.supported(c.nh, c.nkv, c.hd, c.H) != 0;
    }
    // CAKE_ATTN_HEADS=<max keys>[:<waves>]: the head-parallel short-context attention
    if (!ao_ok_ && kvfmt_ == kKv16) {
      const char* e = std::getenv("CAKE_ATTN_HEADS");
      int mx = 0, nw = 2, pfd = 2;
      if (e && *e) std::sscanf(e, "%d:%d:%d", &mx, &nw, &pfd);
      if (mx > 0 && cake_attn_set_heads(mx, nw) == 0 && cake_attn_set_head_prefetch(pfd) == 0)
        heads_max_ = mx;
    }
    if (ao_ok_) {
      ao_ws_ = dalloc<float>((size_t)ao_.ws_floats(c.nkv, c.H));
      const size_t tw = (size_t)ao_.ticket_words(c.nkv, c.H);
      ao_tickets_ = dalloc<unsigned int>(tw);
      hip_check(hipMemset(ao_tickets_, 0, sizeof(unsigned int) * tw), "memset");
    }
    const size_t nseq = 2 * edges_.size() + 2;  // per edge: send, receive sequence
    seq_ = dalloc<unsigned int>(nseq);
    hop_err_ = dalloc<int>(4);
    hip_check(hipMemset(seq_, 0, sizeof(unsigned int) * nseq), "memset");
    hip_check(hipMemset(hop_err_, 0, sizeof(int) * 4), "memset");
    if (tp_ > 1) {
      partial_ = dalloc<float>(c.H);
      ppart_ = dalloc<float>((size_t)S_ * c.H);
      full_logits_ = dalloc<float>(cfg_.V);
      ar_seq_ = dalloc<unsigned int>(8);  // [channel][tag, ticket]
      ar_err_ = dalloc<int>(4);
      hip_check(hipMemset(ar_seq_, 0, sizeof(unsigned int) * 8), "memset");
      hip_check(hipMemset(ar_err_, 0, sizeof(int) * 4), "memset");
    }
    hip_check(hipDeviceSynchronize(), "sync");  // null-stream memsets before st_ work
  }

  // One matrix of 16-bit rows gets its packed twin (m.p13), if K is whole tiles and the copy
  // fits above the HBM reserve (`required`: not fitting is an error); a quantised or absent
  // matrix has no rows to pack.  kind: the row pairing of the GEMV that reads it
  // (cake::PackKind: 0 adjacent rows, 1 head halves, 2 gate | up).
  void pack13_one(int kind, Mat& m, int hd, bool required) {
    constexpr size_t kReserve = (size_t)4 << 30;  // left free for sessions and library workspaces
    const size_t N = m.N, K = m.K;
    if (m.fmt != kFmt16 || !m.w || pack_full_ || K % 2048 != 0) return;
    const int nraw = cake_pack13_rows(kind, m.w, (int)N, (int)K, hd, nullptr, nullptr, nullptr, 0,
                                      st_);
    k_check(nraw < 0 ? -nraw : 0, "pack13_rows (count)");
    const size_t planes = N * (K / 8 * 13), hdrs = (N * 4 + 15) / 16 * 16;
    const size_t bytes = (size_t)cake_pack13_bytes((int)N, (int)K, nraw);
    size_t fr = 0, tot = 0;
    hip_check(hipMemGetInfo(&fr, &tot), "hipMemGetInfo");
    if (fr < bytes + kReserve) {
      if (required)
        throw Error("CAKE_PACK16=1: the packed copy of a [" + std::to_string(N) + ", " +
                    std::to_string(K) + "] matrix (" + std::to_string(bytes >> 20) +
                    " MiB) does not fit above the 4 GiB reserve (" + std::to_string(fr >> 20) +
                    " MiB free)");
      pack_full_ = true;
      return;
    }
    uint8_t* blk = dalloc<uint8_t>(bytes);
    P13Mat p;
    p.planes = blk;
    p.hdr = reinterpret_cast<int*>(blk + planes);
    p.raw = nraw ? reinterpret_cast<uint16_t*>(blk + planes + hdrs) : nullptr;
    const int got = cake_pack13_rows(kind, m.w, (int)N, (int)K, hd, p.planes, p.hdr, p.raw, nraw,
                                     st_);
    k_check(got < 0 ? -got : (got == nraw ? 0 : (int)hipErrorUnknown), "pack13_rows");
    m.p13 = p;
    packed_bytes_ += (int64_t)bytes;
    packed_raw_rows_ += nraw;
    ++packed_mats_;
  }

  // CAKE_PACK16: 0 = off, 1 = required, unset = every matrix that fits (docs/ENV.md);
  // CAKE_PACK16_KINDS: which kinds (qkv,o,gu,down,head; default: those adopted — see
  // profiles/pack13_decode_tuning_sweep.jsonl).  bf16, 16-bit formats, one rank per layer.
  void pack13_all() {
    const char* e = std::getenv("CAKE_PACK16");
    const std::string mode = e ? e : "";
    if (mode == "0") return;
    const bool required = mode == "1";
    if (!mode.empty() && !required) throw Error("CAKE_PACK16 must be 0, 1 or unset, not " + mode);
    if (dt_ != 0 || tp_ > 1) {
      if (required)
        throw Error("CAKE_PACK16=1: the 13-bit packing is of bf16 weights without tensor "
                    "parallelism; unset it (or 0) for f16 and tensor-parallel engines");
      return;
    }
    const char* ke = std::getenv("CAKE_PACK16_KINDS");
    const std::string kinds = "," + std::string(ke && *ke ? ke : kPack13Kinds) + ",";
    struct Entry { const char* name; int kind; Mat* m; int hd; };
    auto pack = [&](std::initializer_list<Entry> entries) {
      for (const Entry& x : entries)
        if (kinds.find("," + std::string(x.name) + ",") != std::string::npos)
          pack13_one(x.kind, *x.m, x.hd, required);
    };
    for (LayerW& w : layers_)
      pack({{"qkv", 1, &w.qkv, lc_.hd}, {"o", 0, &w.o, 0}, {"gu", 2, &w.gu, 0},
            {"down", 0, &w.d, 0}});
    pack({{"head", 0, &lm_head_, 0}});
    std::fprintf(stderr,
                 "cake engine: decode streams %d matrices packed to 13 bits (%d raw rows), "
                 "%.2f GiB beside the 16-bit weights%s (rank %d)\n",
                 packed_mats_, packed_raw_rows_, (double)packed_bytes_ / (double)(1 << 30),
                 pack_full_ ? "; the rest stay 16-bit: HBM reserve reached" : "", rank());
  }

  size_t kv_esize() const { return kvfmt_ == kKvFp8 ? 1 : 2; }  // bytes per cache element
  size_t kv_elems() const { return owned_.size() * (size_t)lc_.nkv * S_ * lc_.hd; }  // of K
  void* kc(int l) const { return cur_.k + (size_t)l * lc_.nkv * S_ * lc_.hd * kv_esize(); }
  void* vc(int l) const { return cur_.v + (size_t)l * lc_.nkv * S_ * lc_.hd * kv_esize(); }

  // KV cache of one session (a master connection of a TCP worker; 0 = generation):
  // allocated on first use, least recently used dropped past kMaxSessions (P4)
  static constexpr size_t kMaxSessions = 8;
  void kv_session(uint64_t id) {
    auto it = kv_.find(id);
    if (it == kv_.end()) {
      if (kv_.size() >= kMaxSessions) {
        uint64_t victim = lru_.front();
        for (uint64_t x : lru_)
          if (x != 0) { victim = x; break; }
        drop_session(victim);
      }
      const size_t n = kv_elems() * kv_esize();
      KV kv{dalloc<uint8_t>(n), dalloc<uint8_t>(n)};
      it = kv_.emplace(id, kv).first;
    }
    lru_.remove(id);
    lru_.push_back(id);
    cur_ = it->second;
  }

 public:
  void drop_session(uint64_t id) {
    auto it = kv_.find(id);
    if (it == kv_.end() || id == 0) return;
    hip_check(hipStreamSynchronize(st_), "sync");
    dfree(it->second.k);
    dfree(it->second.v);
    kv_.erase(it);
    lru_.remove(id);
    if (kv_.count(0)) cur_ = kv_[0];
  }

  // TCP worker compute: `layers` (global indices, this worker's) over hidden [T, H] f32
  // (host, in place) at positions pos0.., with the session's KV cache (worker.rs:236-252;
  // parallel/worker.py _run_ops)
  void forward_host(uint64_t session, const std::vector<int>& layers, int pos0, float* h, int T) {
    hip_check(hipSetDevice(dev_), "hipSetDevice");
    const Cfg& c = lc_;
    if (T < 1 || pos0 < 0 || (int64_t)pos0 + T > S_) throw Error("positions exceed the KV cache");
    std::vector<int> sel;
    for (int l : layers) {
      if (l < 0 || l >= c.L || local_[l] < 0)
        throw Error("layer " + std::to_string(l) + " is not served here");
      sel.push_back(local_[l]);
    }
    kv_session(session);
    if (T == 1) {
      hip_check(hipMemcpyAsync(resid_, h, sizeof(float) * c.H, hipMemcpyHostToDevice, st_), "H2D");
      hip_check(hipMemcpyAsync(pos_, &pos0, sizeof(int), hipMemcpyHostToDevice, st_), "H2D");
      short_step_ = short_at(pos0);
      try {
        step_layers(&sel);
      } catch (...) {
        short_step_ = false;
        throw;
      }
      short_step_ = false;
      hip_check(hipMemcpyAsync(h, resid_, sizeof(float) * c.H, hipMemcpyDeviceToHost, st_), "D2H");
    } else {
      const size_t bytes = sizeof(float) * (size_t)T * c.H;
      hip_check(hipMemcpyAsync(hidden_, h, bytes, hipMemcpyHostToDevice, st_), "H2D");
      prefill_layers(T, pos0, &sel);
      hip_check(hipMemcpyAsync(h, hidden_, bytes, hipMemcpyDeviceToHost, st_), "D2H");
    }
    hip_check(hipStreamSynchronize(st_), "sync");
    if (kv_.count(0)) cur_ = kv_[0];
    if (T == 1) check_attn_error("worker");
  }

 private:
  float scale() const { return 1.0f / std::sqrt((float)cfg_.hd); }

  // an eager step at device position `pos` takes the fused attention + o_proj launch
  // exactly when a one-step graph replay there would (bucket of length pos + 2)
  bool short_at(int pos) const { return short_len(pos + 2); }
  // live lengths served by the cap-1 graph bucket: one split with attention + o_proj fused,
  // or up to heads_max_ keys on the head-parallel attention launch
  bool short_len(int t) const {
    if (ao_ok_) return cake_attn_splits(t) == 1;
    return heads_max_ > 0 && t <= heads_max_;
  }

  // ---- prefill
  void grow_prefill(int T) {
    if (T <= pre_T_) return;
    const Cfg& c = lc_;
    for (void* p : {x16_, qkv_, att_, pact_, (void*)ptok_}) dfree(p);
    const size_t nq = (size_t)c.nh * c.hd, nk = (size_t)c.nkv * c.hd;
    x16_ = dalloc<uint16_t>((size_t)T * c.H);
    qkv_ = dalloc<uint16_t>((size_t)T * (nq + 2 * nk));
    att_ = dalloc<uint16_t>((size_t)T * nq);
    pact_ = dalloc<uint16_t>((size_t)T * c.I);
    ptok_ = dalloc<int32_t>(T);
    if (pfmt_ == 1) {
      dfree(a8_);
      dfree(sa_);
      a8_ = dalloc<uint8_t>((size_t)T * std::max({(size_t)c.H, nq, (size_t)c.I}));
      sa_ = dalloc<float>(T);
    }
    pre_T_ = T;
  }

  void grow_score(int T, int Vc) {
    if (T > sc_T_) {
      for (void* p : {(void*)sc_max_, (void*)sc_sum_, (void*)sc_tgt_, (void*)sc_key_,
                      (void*)sc_lse_, (void*)sc_top_, (void*)sc_topv_, (void*)sc_target_})
        dfree(p);
      sc_max_ = dalloc<float>(T);
      sc_sum_ = dalloc<double>(T);
      sc_tgt_ = dalloc<float>(T);
      sc_key_ = dalloc<unsigned long long>(T);
      sc_lse_ = dalloc<float>(T);
      sc_top_ = dalloc<int32_t>(T);
      sc_topv_ = dalloc<float>(T);
      sc_target_ = dalloc<int32_t>(T);
    }
    if (T > sc_T_ || Vc > sc_Vc_) {
      const int t = std::max(T, sc_T_), v = std::max(Vc, sc_Vc_);
      dfree(sc_logits_);
      sc_logits_ = dalloc<float>((size_t)t * v);
      if (lm_head_.fmt != kFmt16 && v > sc_Vc_) {
        dfree(sc_head_);
        sc_head_ = dalloc<uint16_t>((size_t)v * cfg_.H);
      }
      sc_T_ = t;
      sc_Vc_ = v;
    }
  }

  void gemm(int epi, const void* a, long long lda, const void* b, long long ldb, void* cptr,
            long long ldc, float* resid, long long ldr, int M, int N, int K, const char* what) {
    const bool gated = epi == kEpiSwiglu;
    const long long Nv = gated ? 2LL * N : N;
    static const char* names[] = {"store", "resid32", "add16", "swiglu", "geglu", "partial",
                                  "store32"};
    auto p = planner_.plan(M, Nv, K, names[epi]);
    if (p.first == kGemmLib) {  // the table names the library GEMM (CAKE_GEMM_LIB=1 only)
      if ((epi != kEpiSwiglu || ldc == N) &&
          lib_gemm(epi, a, lda, b, ldb, cptr, ldc, resid, ldr, M, N, K, what))
        return;
      // a strided SwiGLU output or a library failure: the MFMA kernel's plan
      p = planner_.plan_mfma(M, Nv, K, names[epi]);
    }
    const int splits = p.second;
    float* ws = nullptr;
    if (splits > 1) {
      const size_t need = (size_t)cake_gemm_ws_floats(p.first, splits, M, N, K, gated ? 1 : 0);
      if (need > ws_n_) {
        dfree(ws_);
        ws_ = dalloc<float>(need);
        ws_n_ = need;
      }
      ws = ws_;
    }
    k_check(cake_gemm(dt_, epi, p.first, splits, a, lda, b, ldb, cptr, ldc, nullptr, resid, ldr,
                      ws, zeros_, M, N, K, st_), what);
  }

  // hipBLASLt's first call in a process costs ~175 ms (library init; a new shape after it
  // ~0.3 ms: scripts/gpu_runs/gpu_r5_ax.sh): paid here at open, not by the first request's TTFT
  void warm_library() {
    if (!planner_.has_lib()) return;
    if (!lib_ws_) lib_ws_ = dalloc<uint8_t>(kLibWsBytes);
    const size_t n = 64 * 64 + 2 * 8 * 64;  // W [64, 64], A [8, 64], C [8, 64]
    uint16_t* t = dalloc<uint16_t>(n);
    hip_check(hipMemsetAsync(t, 0, n * 2, st_), "memset");
    const int rc = cake_blaslt_gemm(dt_, 0, t + 4096, 64, t, 64, t + 4096 + 512, 64, 8, 64, 64,
                                    lib_ws_, kLibWsBytes, st_);
    hip_check(hipStreamSynchronize(st_), "sync");
    dfree(t);
    if (rc)  // best effort: a library that cannot start leaves every shape on the MFMA kernel
      std::fprintf(stderr, "cake engine: hipBLASLt warm-up failed (rc %d); MFMA GEMMs only\n", rc);
  }

  // store -> 16-bit C; store32 / resid32 -> f32 C with beta 0 / 1; swiglu -> the [M, 2N]
  // product into pgu_, then silu(gate) * up into C.  false (nothing written) when the
  // library refuses the shape: the caller runs the MFMA kernel instead
  bool lib_gemm(int epi, const void* a, long long lda, const void* b, long long ldb, void* cptr,
                long long ldc, float* resid, long long ldr, int M, int N, int K,
                const char* what) {
    if (!lib_ws_) lib_ws_ = dalloc<uint8_t>(kLibWsBytes);
    auto run = [&](int mode, void* c, long long ld, int n) {
      return cake_blaslt_gemm(dt_, mode, a, lda, b, ldb, c, ld, M, n, K, lib_ws_, kLibWsBytes,
                              st_) == 0;
    };
    if (epi == kEpiStore) {
      return run(0, cptr, ldc, N);
    } else if (epi == kEpiStore32 || epi == kEpiResid32) {
      return run(epi == kEpiStore32 ? 1 : 2, resid, ldr, N);
    } else if (epi == kEpiSwiglu && ldc == N) {
      const size_t need = (size_t)M * 2 * N;
      if (need > pgu_n_) {
        dfree(pgu_);
        pgu_ = dalloc<uint16_t>(need);
        pgu_n_ = need;
      }
      if (!run(0, pgu_, 2LL * N, 2 * N)) return false;
      k_check(cake_silu_mul_rows(dt_, pgu_, M, N, cptr, st_), what);
      return true;
    } else {
      throw Error(std::string(what) + ": no library form of this epilogue");
    }
  }

  // embed -> this rank's layers -> (pipeline: the other ranks' layers, hidden rows
  // handed rank to rank through the peers' IPC-mapped prefill buffers) -> head
  void prefill(const int32_t* prompt, int T) {
    prefill_body(prompt, T);
    head_gemv(hidden_ + (size_t)(T - 1) * lc_.H);
  }

  void prefill_body(const int32_t* prompt, int T) {
    const Cfg& c = cfg_;
    if (T > S_) throw Error("prompt longer than max_seq");
    hip_check(hipMemcpyAsync(ptok_buf(T), prompt, sizeof(int32_t) * T, hipMemcpyHostToDevice, st_),
              "prompt H2D");
    k_check(cake_embed(dt_, embed_, ptok_, T, c.H, hidden_, st_), "embed");
    // the walk: rank 0 runs its stops, tells each worker when its stop is due; every
    // stop hands its rows to the next stop's rank (the last one back to this rank)
    for (size_t i = 0; i + 1 < walk_.size(); ++i) {
      const Stop& s = walk_[i];
      if (s.kind == kRemoteStop) {
        remote_rows(s, 0, hidden_, T);
        continue;
      }
      if (s.rank == 0) {
        if (i > 0 && edge_in_[i] >= 0) take_relay(T);  // rows handed back by a worker rank
        if (s.kind == kRunStop) prefill_layers(T, 0, &s.sel);
        if (edge_in_[i + 1] >= 0) forward_hidden(T, walk_[i + 1].rank);
        continue;
      }
      Json m = msg("prefill");
      m.set("T", Json::integer(T));
      m.set("stop", Json::integer((int64_t)i));
      trace(rank_, "prefill stop " + std::to_string(i) + " -> rank " + std::to_string(s.rank));
      ctl_.send(s.rank, m);
      const Json ack = ctl_.recv(s.rank);
      if (!ack.has("ok") || !ack.get("ok").as_bool())
        throw Error("pipeline rank " + std::to_string(s.rank) + " prefill failed: " +
                    (ack.has("error") ? ack.get("error").as_string() : std::string("?")));
    }
    if (edge_in_.back() >= 0) take_relay(T);  // the last worker's rows, for the head
  }

  int32_t* ptok_buf(int T) {
    grow_prefill(T);
    return ptok_;
  }

  // rows [0, T) a peer wrote into this rank's relay buffer -> hidden_ (the copy reads the
  // uncached relay from memory)
  void take_relay(int T) {
    if (!relay_) throw Error("no prefill relay buffer on this rank");
    hip_check(hipMemcpyAsync(hidden_, relay_, sizeof(float) * (size_t)T * cfg_.H,
                             hipMemcpyDeviceToDevice, st_), "prefill relay");
  }

  // hidden_ rows [0, T) -> rank dst's prefill relay buffer (device to device over the IPC
  // mapping), complete before the control message that announces them
  void forward_hidden(int T, int dst) {
    auto it = peer_pbuf_.find(dst);
    if (it == peer_pbuf_.end()) throw Error("no prefill mapping to rank " + std::to_string(dst));
    hip_check(hipMemcpyAsync(it->second, hidden_, sizeof(float) * (size_t)T * cfg_.H,
                             hipMemcpyDeviceToDevice, st_), "prefill hop");
    hip_check(hipStreamSynchronize(st_), "sync");
  }

  void prefill_layers(int T, int pos0 = 0, const std::vector<int>* sel = nullptr) {
    const Cfg& c = lc_;
    grow_prefill(T);
    const int nq = c.nh * c.hd, nk = c.nkv * c.hd, nqkv = nq + 2 * nk;
    const int Tk = pos0 + T;
    const int nl = sel ? (int)sel->size() : (int)layers_.size();
    for (int i = 0; i < nl; ++i) {
      const int l = sel ? (*sel)[i] : i;
      const LayerW& w = layers_[l];
      // one projection GEMM, act [T, K] . m^T.  prefill_fmt 1: the activation rows quantised
      // per token (the weights' own row quantiser over [T, K]), then the fp8 MFMA GEMM on the
      // resident codes: no dequantise pass, the 16-bit scratch untouched.  Else the 16-bit
      // GEMM, on quantised weights (weight_fmt 1, 2) widened into the scratch right before it:
      // one extra pass over the layer's weights per prefill; stream order keeps the four uses
      // of the scratch apart
      auto proj = [&](int epi, const void* act, const Mat& m, void* cptr, long long ldc,
                      float* resid, long long ldr, int N, int K, const char* name) {
        const std::string what = std::string(pfmt_ == 1 ? "gemm_w8a8 " : "gemm ") + name;
        if (pfmt_ != 1)
          return gemm(epi, act, K, dense16(m, 0, m.N, w16_, dt_, st_), K, cptr, ldc, resid, ldr, T,
                      N, K, what.c_str());
        k_check(cake_quant_rows_fp8(dt_, act, T, K, a8_, sa_, st_), "quant_rows_fp8 (activations)");
        k_check(cake_gemm_w8a8(dt_, epi, -1, a8_, K, sa_, m.w, K, m.scale, cptr, ldc, resid, ldr, T,
                               N, K, st_), what.c_str());
      };
      k_check(cake_rmsnorm(dt_, hidden_, w.ln1, (float)c.eps, T, c.H, x16_, st_), "rmsnorm");
      proj(kEpiStore, x16_, w.qkv, qkv_, nqkv, nullptr, 0, nqkv, c.H, "qkv");
      uint16_t* q = reinterpret_cast<uint16_t*>(qkv_);
      // (kv_fmt 0: cake_rope_kv itself)
      k_check(cake_rope_kv_kvf(dt_, q, q + nq, q + nq + nk, nqkv, nqkv, T, c.nh, c.nkv, c.hd,
                               inv_freq_, pos0, S_, kc(l), vc(l), st_, kvfmt_), "rope_kv");
      const void *kr = kc(l), *vr = vc(l);  // what the attention reads
      if (kvfmt_ == kKvFp8) {
        // the live prefix, the rows just written included, widened into the 16-bit scratch:
        // one extra pass over it per layer per prefill call (stream order keeps the layers'
        // uses of the scratch apart)
        k_check(cake_dequant_kv_fp8(dt_, kc(l), vc(l), c.nkv, S_, c.hd, Tk, kv16_k_, kv16_v_,
                                    st_), "dequant_kv_fp8");
        kr = kv16_k_;
        vr = kv16_v_;
      }
      // [B, H, rows, D] strides of q (a column block of qkv), the layer's cache, the output
      const long long Sh = (long long)S_ * c.hd;
      const long long strides[12] = {(long long)T * nqkv, c.hd, nqkv,
                                     (long long)c.nkv * Sh, Sh, c.hd,
                                     (long long)c.nkv * Sh, Sh, c.hd,
                                     (long long)T * nq, c.hd, nq};
      k_check(cake_flash_attn(dt_, q, kr, vr, att_, 1, c.nh, c.nkv, T, Tk, c.hd, strides,
                              scale(), 1, pos0, st_), "flash_attn");
      // tensor parallel: partial o_proj / down_proj over this rank's heads / intermediate
      // range, summed over the ranks
      float* const out = tp_ > 1 ? ppart_ : hidden_;
      const int epi = tp_ > 1 ? kEpiStore32 : kEpiResid32;
      proj(epi, att_, w.o, nullptr, 0, out, c.H, c.H, nq, "o");
      if (tp_ > 1) dense_allreduce(T);
      k_check(cake_rmsnorm(dt_, hidden_, w.ln2, (float)c.eps, T, c.H, x16_, st_), "rmsnorm");
      proj(kEpiSwiglu, x16_, w.gu, pact_, c.I, nullptr, 0, c.I, c.H, "gate|up");
      proj(epi, pact_, w.d, nullptr, 0, out, c.H, c.H, c.I, "down");
      if (tp_ > 1) dense_allreduce(T);
    }
  }

  // ---- token selection / decode step
  Mode mode_of(const CakeEngineSampling& s) const {
    Mode m;
    m.greedy = s.temperature <= 0.f;
    m.penalty = s.repeat_penalty;
    m.last_n = s.repeat_last_n;
    if (!m.greedy) {
      m.temperature = s.temperature;
      m.top_k = s.top_k > 0 ? s.top_k : 0;
      m.top_p = (s.top_p > 0.f && s.top_p < 1.f) ? s.top_p : 0.f;
      m.seed = s.seed;
    }
    m.fused = m.greedy && (m.penalty == 1.f || m.last_n <= kHeadSelectMaxLastN) && tp_ == 1;
    m.logprobs = lp_k_;
    if (lc_next_.on) {  // the controls run in the unfused tail; greedy ignores min_p
      m.min_p = !m.greedy && lc_next_.min_p > 0.f;
      m.controls = m.min_p || lc_next_.presence != 0.f || lc_next_.frequency != 0.f ||
                   !lc_next_.ids.empty();
      if (m.controls) m.fused = false;
    }
    return m;
  }

  // a generation with logit controls starts: the parameter block of lc_next_ (d = T ln min_p
  // formed in f64, rounded once), an empty count table, counted = gen0 = the prompt length
  void lc_begin(int n_prompt, const Mode& m) {
    const LcSetting& c = lc_next_;
    lc_host_.assign(kLcParamWords, 0u);
    auto put = [&](int i, float v) { std::memcpy(&lc_host_[i], &v, 4); };
    put(0, c.presence);
    put(1, c.frequency);
    put(2, m.min_p ? (float)((double)m.temperature * std::log((double)c.min_p)) : 0.f);
    lc_host_[3] = (uint32_t)n_prompt;
    lc_host_[4] = (uint32_t)c.ids.size();
    lc_host_[5] = m.min_p ? 1u : 0u;
    for (size_t i = 0; i < c.ids.size(); ++i) {
      lc_host_[8 + i] = (uint32_t)c.ids[i];
      put(8 + kLcMaxBias + (int)i, c.vals[i]);
    }
    hip_check(hipMemcpyAsync(lc_params_, lc_host_.data(), sizeof(uint32_t) * kLcParamWords,
                             hipMemcpyHostToDevice, st_), "logit controls H2D");
    hip_check(hipMemsetAsync(lc_cnt_, 0, sizeof(unsigned int) * (size_t)lc_.V, st_), "memset");
    hip_check(hipMemsetAsync(lc_state_, 0, sizeof(unsigned int) * kLcStateWords, st_), "memset");
    set_i32(reinterpret_cast<int*>(lc_state_ + 1), n_prompt);
  }

  // the device state one sequence's token selection reads and moves
  struct SelState {
    float* logits;
    int *hist, *hist_len, *tok, *pos;
    unsigned long long* slot;
  };

  // logits -> penalty -> logit controls -> argmax / draw -> finalize (tok, history, pos)
  void select_tail(const Mode& m) { select_tail(m, {logits_, hist_, hist_len_, tok_, pos_, slot_}); }
  void select_tail(const Mode& m, const SelState& s) {
    if (m.penalty != 1.f)
      k_check(cake_repeat_penalty(s.logits, s.hist, s.hist_len, m.last_n, m.penalty, st_), "penalty");
    if (m.controls)  // counts hist_[counted, hist_len) first: before finalize moves hist_len
      k_check(cake_logit_controls(s.logits, lc_.V, s.hist, s.hist_len, lc_cnt_, lc_params_, lc_state_,
                                  0, st_), "logit_controls");
    if (m.greedy) {
      k_check(cake_argmax(s.logits, lc_.V, s.slot, st_), "argmax");
    } else {
      const bool restrict = m.top_k > 0 || m.top_p > 0.f;
      if (restrict)
        k_check(cake_sample_threshold(s.logits, lc_.V, m.temperature, m.top_k, m.top_p, thr_, st_),
                "sample_threshold");
      const unsigned int* thr = restrict ? thr_ : nullptr;
      if (m.min_p) {  // the sets intersect: the larger key
        if (restrict) k_check(cake_logit_controls_merge_thr(thr_, lc_state_ + 2, st_), "merge_thr");
        else thr = lc_state_ + 2;
      }
      k_check(cake_gumbel_argmax(s.logits, lc_.V, m.temperature, m.seed, s.hist_len, thr, s.slot,
                                 st_), "gumbel_argmax");
    }
    k_check(cake_finalize_token(s.slot, s.tok, s.hist, s.hist_len, s.pos, S_, st_), "finalize");
  }

  // the record of the token just finalised: logits_ still holds the row selection saw (the
  // penalised values on every path), tok_ and hist_len_ the new values
  void logprob_record(const Mode& m) {
    if (m.logprobs < 0) return;
    k_check(cake_logprob_topk(logits_, lc_.V, tok_, hist_len_, m.logprobs, lp_rec_, S_, lp_ws_,
                              lp_ticket_, 0, st_), "logprob_topk");
  }

  // one decode step of this rank: its stops of the walk in order — receive (when the
  // previous stop is another rank's), the stop's work (embedding / layer run / head),
  // send (when the next stop is another rank's); the hop carries [hidden | position]
  void step_body(const Mode& m) {
    for (size_t i = 0; i < walk_.size(); ++i) {
      const Stop& s = walk_[i];
      if (s.rank != rank_) continue;
      if (edge_in_[i] >= 0) hop_recv(edge_in_[i]);
      if (s.kind == kEmbedStop) {
        if (!m.fused) k_check(cake_embed(dt_, embed_, tok_, 1, cfg_.H, resid_, st_), "embed");
      } else if (s.kind == kRunStop) {
        step_layers(&s.sel);
      } else if (s.kind == kRemoteStop) {
        remote_step(s);
      } else {
        step_head(m);
      }
      if (i + 1 < walk_.size() && edge_in_[i + 1] >= 0) hop_send(edge_in_[i + 1]);
    }
  }

  bool has_stops() const {
    for (const Stop& s : walk_)
      if (s.rank == rank_) return true;
    return false;
  }

  void hop_send(int e) {
    k_check(cake_hop_send(resid_, cfg_.H, 1, hop_bf16_ ? 1 : 0, out_inbox_.at(e), seq_ + 2 * e, st_),
            "hop_send");
  }
  void hop_recv(int e) {
    k_check(cake_hop_recv(my_inbox_.at(e), cfg_.H, 1, hop_bf16_ ? 1 : 0, resid_, seq_ + 2 * e + 1,
                          hop_err_, hop_timeout_, st_), "hop_recv");
  }

  // the walk of one token over the owner map (the placement loop llama.rs:205-220 and
  // the contiguous-run coalescing of llama.rs:95-114)
  void plan_walk() {
    walk_.clear();
    walk_.push_back({kEmbedStop, 0, {}, {}});
    for (int l = 0; l < cfg_.L; ++l) {
      const int w = remote_of_.empty() ? -1 : remote_of_[l];
      if (w >= 0) {  // a TCP worker's run: coalesced while the worker stays the same
        if (walk_.back().kind != kRemoteStop || walk_.back().remote != w)
          walk_.push_back({kRemoteStop, 0, {}, {}, w});
        walk_.back().layers.push_back(l);
        continue;
      }
      const int r = owner_.empty() ? 0 : owner_[l];
      if (walk_.back().kind != kRunStop || walk_.back().rank != r) walk_.push_back({kRunStop, r, {}, {}});
      walk_.back().layers.push_back(l);
      if (r == rank_) walk_.back().sel.push_back(local_[l]);
    }
    walk_.push_back({kHeadStop, 0, {}, {}});
    edge_in_.assign(walk_.size(), -1);
    edges_.clear();
    for (size_t i = 1; i < walk_.size(); ++i)
      if (walk_[i].rank != walk_[i - 1].rank) {
        edge_in_[i] = (int)edges_.size();
        edges_.push_back({walk_[i - 1].rank, walk_[i].rank});
      }
  }

 public:
  // "r:l0-l1,..." of the walk (logs / tests)
  std::string walk_str() const {
    std::string s;
    for (const Stop& st : walk_)
      if (st.kind == kRunStop || st.kind == kRemoteStop) {
        if (!s.empty()) s += ",";
        s += (st.kind == kRemoteStop ? "w" + std::to_string(st.remote) : std::to_string(st.rank)) +
             ":" + std::to_string(st.layers.front()) + "-" + std::to_string(st.layers.back());
      }
    return s;
  }
  int n_edges() const { return (int)edges_.size(); }

 private:

  // decode attention of local layer l into attn_out_: over the fp8 code cache (kv_fmt 1),
  // head-parallel for a short context, split over the context otherwise
  void attn(int l) { attn(l, q_, pos_, attn_out_); }
  void attn(int l, const float* q, const int* pos, void* out) {
    const Cfg& c = lc_;
    if (kvfmt_ == kKvFp8)
      k_check(cake_attn_decode_kv8(dt_, q, kc(l), vc(l), pos, S_, c.nh, c.nkv, c.hd, scale(),
                                   part_, tickets_, out, st_), "attn_decode_kv8");
    else if (short_step_)
      k_check(cake_attn_decode_heads(dt_, q, kc(l), vc(l), pos, S_, c.nh, c.nkv, c.hd,
                                     scale(), out, st_), "attn_heads");
    else
      k_check(cake_attn_decode(dt_, q, kc(l), vc(l), pos, S_, c.nh, c.nkv, c.hd, scale(),
                               part_, tickets_, out, st_), "attn_decode");
  }

  // every GEMV through its dispatcher (llama_weights.h: the entry point of the matrix's format
  // or packed twin); tensor parallel: o_proj / down_proj partial sums, summed over the ranks
  void step_layers(const std::vector<int>* sel = nullptr) {
    const Cfg& c = lc_;
    const int nq = c.nh * c.hd;
    const int nl = sel ? (int)sel->size() : (int)layers_.size();
    float* const out = tp_ > 1 ? partial_ : resid_;
    const int accumulate = tp_ > 1 ? 0 : 1;
    for (int i = 0; i < nl; ++i) {
      const int l = sel ? (*sel)[i] : i;
      const LayerW& w = layers_[l];
      k_check(qkv_rope(dt_, resid_, w.ln1, (float)c.eps, w.qkv, c.H, c.nh, c.nkv, c.hd, inv_freq_,
                       pos_, q_, kc(l), vc(l), S_, st_, kvfmt_), "qkv_rope", w.qkv);
      if (kvfmt_ != kKvFp8 && short_step_ && ao_ok_) {  // one split: attention + o_proj fused
        k_check(ao_.run(dt_, q_, kc(l), vc(l), pos_, S_, c.nh, c.nkv, c.hd, scale(), w.o.w, nq, c.H,
                        out, accumulate, ao_ws_, ao_tickets_, tickets_ + 2 * c.nkv, st_),
                "attn_oproj");
      } else {  // (the fp8 cache runs with tp_ == 1)
        attn(l);
        k_check(gemv_x16(dt_, attn_out_, w.o, nq, c.H, out, accumulate, st_), "o_proj", w.o);
      }
      if (tp_ > 1) ar_sum();
      k_check(swiglu(dt_, resid_, w.ln2, (float)c.eps, w.gu, c.H, c.I, act_, st_), "swiglu", w.gu);
      k_check(gemv_x16(dt_, act_, w.d, c.I, c.H, out, accumulate, st_), "down_proj", w.d);
      if (tp_ > 1) ar_sum();
    }
  }

  // ---- lock-step batched decode
  void batch_alloc(int B) {
    const Cfg& c = lc_;
    const size_t nq = (size_t)c.nh * c.hd, nk = (size_t)c.nkv * c.hd, R = kMaxBatch;
    if (!b_.resid) {
      b_.resid = dalloc<float>(R * c.H);
      b_.qkv32 = dalloc<float>(R * (nq + 2 * nk));
      b_.q = dalloc<float>(R * nq);
      b_.logits = dalloc<float>(R * c.V);
      b_.logits2 = dalloc<float>(2 * R * c.V);
      b_.x16 = dalloc<uint16_t>(2 * R * c.H);
      b_.attn = dalloc<uint16_t>(R * nq);
      b_.act = dalloc<uint16_t>(R * c.I);
      b_.tok = dalloc<int>(R);
      b_.pos = dalloc<int>(R);
      b_.hist = dalloc<int>(R * S_);
      b_.hist_len = dalloc<int>(R);
      b_.slot = dalloc<unsigned long long>(R);
      b_.kbase = dalloc<void*>(R);
      b_.vbase = dalloc<void*>(R);
      hip_check(hipHostMalloc(reinterpret_cast<void**>(&b_.host_tok), sizeof(int32_t) * 2 * R,
                              hipHostMallocDefault), "hipHostMalloc");
    }
    while ((int)b_.kv.size() < B) {
      const size_t n = kv_elems() * kv_esize();
      b_.kv.push_back(KV{dalloc<uint8_t>(n), dalloc<uint8_t>(n)});
    }
    std::vector<void*> kb(R, nullptr), vb(R, nullptr);
    for (size_t b = 0; b < b_.kv.size(); ++b) {
      kb[b] = b_.kv[b].k;
      vb[b] = b_.kv[b].v;
    }
    hip_check(hipMemcpyAsync(b_.kbase, kb.data(), sizeof(void*) * R, hipMemcpyHostToDevice, st_),
              "kbase H2D");
    hip_check(hipMemcpyAsync(b_.vbase, vb.data(), sizeof(void*) * R, hipMemcpyHostToDevice, st_),
              "vbase H2D");
    hip_check(hipStreamSynchronize(st_), "sync");
  }

  // one step of B rows: token index i of every sequence (device position T[b] + i - 1), up to
  // the [B, V] logits; the caller selects
  void batch_step(int B, const std::vector<int>& T, int i) {
    const Cfg& c = lc_;
    const int nq = c.nh * c.hd, nqkv = nq + 2 * c.nkv * c.hd;
    const float eps = (float)c.eps;
    auto rows = [&](int epi, const void* x, int K, const Mat& m, void* o, long long ldo,
                    float* resid, int N, const char* what) {
      k_check(cake_gemv_rows(dt_, epi, x, K, m.w, K, o, ldo, resid, resid ? N : 0, B, N, K, st_),
              what);
    };
    k_check(cake_embed(dt_, embed_, b_.tok, B, c.H, b_.resid, st_), "embed");
    for (size_t l = 0; l < layers_.size(); ++l) {
      const LayerW& w = layers_[l];
      k_check(cake_rmsnorm(dt_, b_.resid, w.ln1, eps, B, c.H, b_.x16, st_), "rmsnorm");
      rows(kEpiStore32, b_.x16, c.H, w.qkv, b_.qkv32, nqkv, nullptr, nqkv, "gemv_rows qkv");
      k_check(cake_rope_kv_rows(dt_, b_.qkv32, nqkv, B, b_.pos, inv_freq_, c.nh, c.nkv, c.hd, S_,
                                b_.q, b_.kbase, b_.vbase, (long long)l * c.nkv * S_ * c.hd, st_),
              "rope_kv_rows");
      for (int b = 0; b < B; ++b) {  // the launch a batch-1 step picks at this sequence's length
        cur_ = b_.kv[b];
        short_step_ = heads_max_ > 0 && short_at(T[b] + i - 1);
        attn((int)l, b_.q + (size_t)b * nq, b_.pos + b, b_.attn + (size_t)b * nq);
      }
      short_step_ = false;
      rows(kEpiResid32, b_.attn, nq, w.o, nullptr, 0, b_.resid, c.H, "gemv_rows o_proj");
      k_check(cake_rmsnorm(dt_, b_.resid, w.ln2, eps, B, c.H, b_.x16, st_), "rmsnorm");
      rows(kEpiSwiglu, b_.x16, c.H, w.gu, b_.act, c.I, nullptr, c.I, "gemv_rows gate|up");
      rows(kEpiResid32, b_.act, c.I, w.d, nullptr, 0, b_.resid, c.H, "gemv_rows down_proj");
    }
    // the head on the f32 normalised rows as two 16-bit terms each (the batch-1 head reads
    // them in f32): 2B rows on one pass over the head, then the two f32 sums added
    k_check(cake_rmsnorm_split_rows(dt_, b_.resid, norm_, eps, B, c.H, b_.x16, st_),
            "rmsnorm_split_rows");
    k_check(cake_gemv_rows(dt_, kEpiStore32, b_.x16, c.H, lm_head_.w, c.H, b_.logits2, c.V, nullptr,
                           0, 2 * B, c.V, c.H, st_), "gemv_rows lm_head");
    k_check(cake_sum_slices(b_.logits, b_.logits2, 2, (long long)B * c.V, (long long)B * c.V, 0,
                            st_), "sum_slices");
  }

  void step_head(const Mode& m) {
    const Cfg& c = lc_;
    if (forced_) {  // teacher forcing: the full logits, no token choice
      head_logits(resid_);
      return;
    }
    if (tp_ > 1) {
      head_tp(resid_, m);
      return;
    }
    if (m.fused) {
      const int last_n = m.penalty != 1.f ? m.last_n : 0;
      k_check(head_select(dt_, resid_, norm_, (float)c.eps, lm_head_, c.H, c.V, logits_, hist_,
                          hist_len_, last_n, m.penalty, slot_, sel_ticket_, tok_, pos_, S_, embed_,
                          resid_, st_), "head_select", lm_head_);
      logprob_record(m);
      return;
    }
    head_gemv(resid_);
    select_tail(m);
    logprob_record(m);
  }

  // logits_ = lm_head . rms_norm(row): the 16-bit head, its packed or its quantised twin
  void head_gemv(const float* row) {
    const Cfg& c = lc_;
    k_check(gemv_norm_f32(dt_, row, norm_, (float)c.eps, lm_head_, c.H, c.V, logits_, st_),
            "lm_head", lm_head_);
  }

  // f32 logits of the whole vocabulary for one hidden row: logits_ (one rank), or this
  // rank's vocabulary shard gathered into full_logits_ on every tensor-parallel rank
  float* head_logits(const float* row) {
    const Cfg& c = lc_;
    head_gemv(row);
    if (tp_ == 1) return logits_;
    k_check(cake_ar_gather(logits_, voff_, c.V, full_logits_, cfg_.V, ch_gat_.peers.data(),
                           ch_gat_.inbox, ar_seq_ + 4, ar_err_ + 2, tp_rank_, tp_, hop_timeout_,
                           st_), "ar_gather");
    return full_logits_;
  }

  // Teacher forcing: prefill `prompt`, then feed forced[0..n) one decode step each
  // (eager launches of the same decode kernels, hops and all-reduces as the captured
  // step); out[(n + 1) x V] = the logits after the prompt and after every forced token.
  // Rank 0 drives; pipeline workers run their stops on "fstep", tensor-parallel workers
  // the whole sequence on "forced".
  void forced_run(const int32_t* prompt, int T, const int32_t* forced, int n, float* out) {
    const bool lead = rank_ == 0 && tp_rank_ == 0;
    grow_prefill(T);
    if (tp_ > 1 && lead) {
      Json m = msg("forced");
      Json pr = Json::array(), fr = Json::array();
      for (int i = 0; i < T; ++i) pr.push(Json::integer(prompt[i]));
      for (int i = 0; i < n; ++i) fr.push(Json::integer(forced[i]));
      m.set("prompt", pr);
      m.set("forced", fr);
      ctl_.broadcast(m);
    }
    prefill_body(prompt, T);
    const size_t V = cfg_.V;
    float* lg = head_logits(hidden_ + (size_t)(T - 1) * cfg_.H);
    if (out) hip_check(hipMemcpyAsync(out, lg, sizeof(float) * V, hipMemcpyDeviceToHost, st_), "D2H");
    hip_check(hipStreamSynchronize(st_), "sync");
    Mode m;
    m.fused = false;
    forced_ = true;
    try {
      for (int i = 0; i < n; ++i) {
        if (world_ > 1) {
          Json st = msg("fstep");
          st.set("pos", Json::integer(T + i));
          ctl_.broadcast(st);
        }
        set_i32(tok_, forced[i]);
        set_i32(pos_, T + i);
        short_step_ = short_at(T + i);
        step_body(m);
        short_step_ = false;
        if (out)
          hip_check(hipMemcpyAsync(out + (size_t)(i + 1) * V, tp_ > 1 ? full_logits_ : logits_,
                                   sizeof(float) * V, hipMemcpyDeviceToHost, st_), "D2H");
        hip_check(hipStreamSynchronize(st_), "sync");
      }
    } catch (...) {
      forced_ = false;
      short_step_ = false;
      throw;
    }
    forced_ = false;
    if (world_ > 1) sync_workers(hop_drain());
    if (tp_ > 1 && lead) sync_workers(ar_drain());
    if (lead) check_attn_error("rank " + std::to_string(rank()));
  }

  // ---- TCP workers (master side; the reference's Client, client.rs:23-133)
  void connect_remotes() {
    for (auto& w : remotes_) {
      std::string host;
      int port = 0;
      split_host_port(w.addr, &host, &port);
      w.fd = tcp_connect(host, port, remote_timeout_);
      tcp_set_timeout(w.fd, remote_timeout_);
      Message hello;
      hello.type = MsgType::Hello;
      const std::string body = encode_body(hello);
      send_frame(w.fd, reinterpret_cast<const uint8_t*>(body.data()), (uint32_t)body.size());
      const std::string rep = recv_frame(w.fd);
      const Message info = decode_body(reinterpret_cast<const uint8_t*>(rep.data()), rep.size());
      if (info.type != MsgType::WorkerInfo)
        throw Error("worker " + w.addr + " did not answer Hello with WorkerInfo");
      trace(0, "worker " + w.addr + ": " + info.info.device + " " + info.info.dtype + " (" +
                   info.info.os + "/" + info.info.arch + "), handshake " +
                   std::to_string(info.info.latency_lo) + " ms");
    }
  }

  static float wire_to_f32(uint16_t h, bool bf16) {
    uint32_t bits;
    if (bf16) {
      bits = (uint32_t)h << 16;
    } else {
      const uint32_t sg = (uint32_t)(h & 0x8000) << 16, e = (h >> 10) & 0x1f, m = h & 0x3ff;
      if (e == 0) {
        if (m == 0) {
          bits = sg;
        } else {
          int ee = -1;
          uint32_t mm = m;
          do { ++ee; mm <<= 1; } while (!(mm & 0x400));
          bits = sg | ((uint32_t)(127 - 15 - ee) << 23) | ((mm & 0x3ff) << 13);
        }
      } else if (e == 31) {
        bits = sg | 0x7f800000u | (m << 13);
      } else {
        bits = sg | ((e + 127 - 15) << 23) | (m << 13);
      }
    }
    float f;
    std::memcpy(&f, &bits, 4);
    return f;
  }

  // one Batch round trip: host_rows_ [T, H] f32 at positions pos0.. through the worker's
  // run of layers (one (model.layers.l, pos0, l) item per layer), replaced by the reply
  void remote_call(const Stop& s, int pos0, int T) {
    RemoteWorker& w = remotes_.at(s.remote);
    const size_t n = (size_t)T * cfg_.H;
    Message m;
    m.type = MsgType::Batch;
    m.x.dtype = "f32";
    m.x.shape = {1, (uint64_t)T, (uint64_t)cfg_.H};
    m.x.data = reinterpret_cast<const uint8_t*>(host_rows_.data());
    m.x.nbytes = n * 4;
    for (int l : s.layers)
      m.batch.push_back({"model.layers." + std::to_string(l), (uint64_t)pos0, (uint64_t)l});
    const std::string body = encode_body(m);
    send_frame(w.fd, reinterpret_cast<const uint8_t*>(body.data()), (uint32_t)body.size());
    const std::string rep = recv_frame(w.fd);
    const Message r = decode_body(reinterpret_cast<const uint8_t*>(rep.data()), rep.size());
    if (r.type == MsgType::Error) throw Error("worker " + w.addr + ": " + r.error);
    if (r.type != MsgType::Tensor) throw Error("worker " + w.addr + ": unexpected reply");
    uint64_t cnt = 1;
    for (auto d : r.x.shape) cnt *= d;
    if (cnt != n) throw Error("worker " + w.addr + ": reply of " + std::to_string(cnt) +
                              " values, expected " + std::to_string(n));
    if (r.x.dtype == "f32" && r.x.nbytes == n * 4) {
      std::memcpy(host_rows_.data(), r.x.data, n * 4);
    } else if ((r.x.dtype == "f16" || r.x.dtype == "bf16") && r.x.nbytes == n * 2) {
      const bool bf = r.x.dtype == "bf16";
      for (size_t i = 0; i < n; ++i) {
        uint16_t h;
        std::memcpy(&h, r.x.data + 2 * i, 2);
        host_rows_[i] = wire_to_f32(h, bf);
      }
    } else {
      throw Error("worker " + w.addr + ": unsupported reply tensor " + r.x.dtype);
    }
  }

  // prefill rows [T, H] (device) through a remote run
  void remote_rows(const Stop& s, int pos0, float* rows, int T) {
    const size_t n = (size_t)T * cfg_.H;
    host_rows_.resize(n);
    hip_check(hipMemcpyAsync(host_rows_.data(), rows, n * 4, hipMemcpyDeviceToHost, st_), "D2H");
    hip_check(hipStreamSynchronize(st_), "sync");
    remote_call(s, pos0, T);
    hip_check(hipMemcpyAsync(rows, host_rows_.data(), n * 4, hipMemcpyHostToDevice, st_), "H2D");
    hip_check(hipStreamSynchronize(st_), "sync");
  }

  // the decode row through a remote run; its position rides in resid_'s header word
  void remote_step(const Stop& s) {
    const int H = cfg_.H;
    host_rows_.resize((size_t)H + 1);
    hip_check(hipMemcpyAsync(host_rows_.data(), resid_, sizeof(float) * (H + 1),
                             hipMemcpyDeviceToHost, st_), "D2H");
    hip_check(hipStreamSynchronize(st_), "sync");
    int pos = 0;
    std::memcpy(&pos, &host_rows_[H], 4);
    remote_call(s, pos, 1);
    hip_check(hipMemcpyAsync(resid_, host_rows_.data(), sizeof(float) * H, hipMemcpyHostToDevice,
                             st_), "H2D");
    hip_check(hipStreamSynchronize(st_), "sync");
  }

  // decode with TCP workers in the walk: every step eagerly (host round trips inside it),
  // the token read back after each; per-token host wall time
  int decode_eager(int pos0, int n, const Mode& m, const int32_t* eos, int n_eos,
                   cake_engine_token_cb cb, void* ctx, int32_t* out, int out_cap,
                   std::vector<float>* ms_out) {
    std::vector<float> ms;
    int n_out = 0;
    for (int i = 0; i < n; ++i) {
      const auto t0 = std::chrono::steady_clock::now();
      short_step_ = short_at(pos0 + i);
      try {
        step_body(m);
      } catch (...) {
        short_step_ = false;
        throw;
      }
      short_step_ = false;
      int32_t tok = 0;
      hip_check(hipMemcpyAsync(&tok, tok_, sizeof(tok), hipMemcpyDeviceToHost, st_), "tok");
      if (lp_on_) {  // the step's record: history index pos + 1 = pos0 + i + 1
        if ((size_t)(lp_n_ + 1) * kLpRecWords > lp_host_.size()) throw Error("log-prob copy overrun");
        int32_t hl = 0;
        hip_check(hipMemcpyAsync(&hl, hist_len_, sizeof(hl), hipMemcpyDeviceToHost, st_), "len");
        hip_check(hipStreamSynchronize(st_), "sync");
        if (hl < 1 || hl > S_) throw Error("log-probs: history length out of range");
        hip_check(hipMemcpyAsync(lp_host_.data() + (size_t)lp_n_ * kLpRecWords,
                                 lp_rec_ + (size_t)(hl - 1) * kLpRecWords, kLpRecWords * 4,
                                 hipMemcpyDeviceToHost, st_), "logprob D2H");
      }
      hip_check(hipStreamSynchronize(st_), "sync");
      if (lp_on_) ++lp_n_;
      ms.push_back((float)(std::chrono::duration<double>(std::chrono::steady_clock::now() - t0)
                               .count() * 1e3));
      if (n_out < out_cap) out[n_out++] = tok;
      bool stop = cb && cb(ctx, tok) != 0;
      for (int e = 0; e < n_eos && !stop; ++e)
        if (eos[e] == tok) stop = true;
      if (stop) break;
    }
    check_attn_error("rank 0");
    if (ms_out) *ms_out = std::move(ms);
    return n_out;
  }

  bool remote_mode() const { return !remotes_.empty(); }

  // ---- pipeline (one process per GPU, layer shards, device-side hops)
  static constexpr int kAnnounceChunk = 8;  // replays per worker announcement
  struct AnnounceCtx {
    Llama* self;
    int pos0;  // device position before the first replay of this run
  };
  static int32_t announce_cb(void* vctx, int32_t first, int32_t count) {
    auto* a = static_cast<AnnounceCtx*>(vctx);
    try {
      Json m = msg("replays");
      m.set("count", Json::integer(count));
      m.set("pos", Json::integer(a->pos0 + (int64_t)first * a->self->k_));
      a->self->ctl_.broadcast(m);
      return 0;
    } catch (const std::exception&) {
      return 1;
    }
  }

  // The device-side waits of a mode and how its drain names them: the error words a wait
  // that gave up sets, their key in a worker's "sync" reply, and the texts.
  struct Drain {
    int* err;
    int words;
    const char *key, *label, *what;
  };
  Drain hop_drain() const {
    return {hop_err_, 1, "hop_err", "pipeline rank ", "hop receive timed out"};
  }
  Drain ar_drain() const {
    return {ar_err_, 3, "ar_err", "tensor-parallel rank ", "all-reduce timed out"};
  }

  // this rank's error words, read and reset (a worker reports what it can: unchecked)
  static int take_errors(const Drain& d, bool checked) {
    int w[3] = {0, 0, 0};
    const hipError_t e = hipMemcpy(w, d.err, sizeof(int) * d.words, hipMemcpyDeviceToHost);
    if (checked) hip_check(e, d.key);
    if (w[0] | w[1] | w[2]) (void)hipMemset(d.err, 0, sizeof(int) * d.words);
    return w[0] | w[1] | w[2];
  }

  // rank 0: every worker drained its stream; any wait that gave up is an error
  void sync_workers(const Drain& d) {
    std::string err;
    for (int r = 1; r <= ctl_.workers(); ++r) {
      try {
        ctl_.send(r, msg("sync"));
        const Json j = ctl_.recv(r);
        const std::string who = d.label + std::to_string(r) + ": ";
        if (j.has(d.key) && j.get(d.key).as_int() != 0) err = who + d.what;
        if (j.has("error")) err = (tp_ > 1 ? "" : who) + j.get("error").as_string();
      } catch (const std::exception& e) {
        err = e.what();
      }
    }
    if (take_errors(d, true)) err =std::string(d.label) + "0: " + d.what;
    if (!err.empty()) throw Error(err);
  }

  // a worker's answer to "sync": its stream drained, its error words, what went wrong
  void reply_sync(const Drain& d) {
    Json r = Json::object();
    const hipError_t e = hipStreamSynchronize(st_);
    r.set("ok", Json::boolean(e == hipSuccess));
    r.set(d.key, Json::integer(take_errors(d, false)));
    if (e != hipSuccess) r.set("error", Json::string(hipGetErrorString(e)));
    try {  // pipeline: rank 0 names the rank before whatever this reports
      check_attn_error(tp_ > 1 ? d.label + std::to_string(tp_rank_) : "attention");
    } catch (const std::exception& x) {
      r.set("error", Json::string(x.what()));
    }
    ctl_.send(0, r);
  }

 public:
  // worker rank: serve the master's control messages until it says exit
  void serve() {
    hip_check(hipSetDevice(dev_), "hipSetDevice");
    if (tp_ > 1) {
      if (tp_rank_ == 0) throw Error("serve() runs on tensor-parallel workers (rank > 0)");
      serve_tp();
      return;
    }
    if (head_) throw Error("serve() runs on pipeline workers (rank > 0)");
    const bool active = has_stops();  // a rank the placement left idle only answers
    if (active) ensure_graphs(Mode{});
    std::vector<void*> execs(execs_.begin(), execs_.end());
    for (;;) {
      const Json m = ctl_.recv(0);
      const std::string cmd = m.get("cmd").as_string();
      trace(rank_, "control: " + m.dump().substr(0, 120));
      if (cmd == "exit") break;
      if (cmd == "prefill") {
        Json r = Json::object();
        try {
          const int T = (int)m.get("T").as_int();
          const int i = (int)m.get("stop").as_int();
          if (T < 1 || T > S_) throw Error("bad prefill length");
          if (i < 1 || i + 1 >= (int)walk_.size() || walk_[i].rank != rank_)
            throw Error("prefill stop " + std::to_string(i) + " is not this rank's");
          if (edge_in_[i] >= 0) take_relay(T);
          prefill_layers(T, 0, &walk_[i].sel);
          if (edge_in_[i + 1] >= 0) forward_hidden(T, walk_[i + 1].rank);
          r.set("ok", Json::boolean(true));
        } catch (const std::exception& e) {
          r.set("ok", Json::boolean(false));
          r.set("error", Json::string(e.what()));
        }
        ctl_.send(0, r);
      } else if (cmd == "fstep") {  // one eager teacher-forced step of this rank's stops
        if (!active) continue;
        Mode fm;
        fm.fused = false;
        short_step_ = short_at((int)m.get("pos").as_int());
        step_body(fm);
        short_step_ = false;
      } else if (cmd == "replays") {
        if (!active) continue;
        CakeLoopSpec spec{};
        spec.execs = execs.data();
        spec.n_execs = (int32_t)execs.size();
        spec.bucket_of = bucket_of_.data();
        spec.n_len = (int32_t)bucket_of_.size();
        spec.k = k_;
        spec.pos = (int32_t)m.get("pos").as_int();
        spec.n = (int32_t)m.get("count").as_int() * k_;
        spec.stream = st_;
        CakeLoopResult res{};
        k_check(cake_graph_decode(&spec, &res), "graph_decode");  // enqueue only
      } else if (cmd == "sync") {
        reply_sync(hop_drain());
      } else {
        throw Error("unknown control message " + cmd);
      }
    }
  }

 private:
  // inboxes (uncached device memory, device-side hops) and prefill buffers exchanged as
  // IPC handles over the TCP control plane; ring: rank r sends to (r + 1) % world
  void connect_pipeline(const std::string& addr, double timeout_s) {
    const int words = cake_hop_words(cfg_.H, 1, hop_bf16_ ? 1 : 0);
    // this rank's handles: its prefill buffer and one inbox per edge into it
    Json me = Json::object();
    void* rp = nullptr;
    k_check(cake_hop_alloc(sizeof(float) * (size_t)S_ * cfg_.H, &rp), "relay alloc");
    relay_ = static_cast<float*>(rp);
    me.set("pbuf", Json::string(ipc_export(relay_)));
    Json ib = Json::array();
    for (size_t e = 0; e < edges_.size(); ++e) {
      if (edges_[e].second != rank_) continue;
      void* p = nullptr;
      k_check(cake_hop_alloc((size_t)words * 8, &p), "hop_alloc");
      my_inbox_[(int)e] = p;
      Json x = Json::array();
      x.push(Json::integer((int64_t)e));
      x.push(Json::string(ipc_export(p)));
      ib.push(x);
    }
    me.set("inboxes", ib);
    ctl_.open(addr, rank_, world_, me, timeout_s, "bad pipeline rank hello");
    // map the receivers of this rank's outgoing edges: their inbox, their prefill buffer
    for (size_t e = 0; e < edges_.size(); ++e) {
      if (edges_[e].first != rank_) continue;
      const int dst = edges_[e].second;
      const Json& t = ctl_.table()[dst];
      bool found = false;
      for (const auto& x : t.get("inboxes").items()) {
        if ((int)x.at(0).as_int() != (int)e) continue;
        out_inbox_[(int)e] = ipc_import(x.at(1).as_string(), "IpcOpen inbox");
        found = true;
      }
      if (!found) throw Error("rank " + std::to_string(dst) + " published no inbox for edge " +
                              std::to_string(e));
      if (!peer_pbuf_.count(dst))
        peer_pbuf_[dst] = ipc_import(t.get("pbuf").as_string(), "IpcOpen pbuf");
    }
  }

  // Start-up self-test of every edge (before any graph exists): each rank pushes a
  // tagged pattern through each outgoing edge (non-blocking peer stores), then receives
  // on each incoming edge (bounded device wait) and checks every word; every rank's
  // verdict goes to rank 0, which fails the start with the rank and peer named.  A
  // mapping that does not carry stores across the devices fails here, not as a hop
  // timeout in the middle of the first generation.
  static float selftest_value(int e, int i) { return (float)(((i * 7 + e * 13) % 251) - 125); }

  static bool selftest_forced_fail() {  // test hook: the fallback path of bench / cake-cli
    const char* e = std::getenv("CAKE_IPC_SELFTEST_FAIL");
    return e && *e == '1';
  }

  // Each outgoing edge writes a pattern row into the receiver's relay buffer the way
  // forward_hidden does (device copy over the IPC mapping, synchronized before the
  // control message); after a barrier the receiver moves it out with take_relay's copy
  // and checks every word.  Round 2 writes a new pattern over rows the receiver has
  // already read, so a receiver that kept the old contents in a cache fails here.
  void selftest_relay(std::string& bad) {
    const int H = cfg_.H;
    std::vector<float> pat(H), got(H);
    for (int round = 1; round <= 2; ++round) {
      for (size_t e = 0; e < edges_.size(); ++e) {
        if (edges_[e].first != rank_ || (int)e >= S_) continue;
        for (int i = 0; i < H; ++i) pat[i] = selftest_value((int)e + 64 * round, i);
        hip_check(hipMemcpyAsync(hidden_, pat.data(), sizeof(float) * H, hipMemcpyHostToDevice,
                                 st_), "selftest H2D");
        float* dst = static_cast<float*>(peer_pbuf_.at(edges_[e].second)) + e * (size_t)H;
        hip_check(hipMemcpyAsync(dst, hidden_, sizeof(float) * H, hipMemcpyDeviceToDevice, st_),
                  "selftest relay");
        hip_check(hipStreamSynchronize(st_), "selftest sync");
      }
      ctl_.barrier();
      for (size_t e = 0; e < edges_.size(); ++e) {
        if (edges_[e].second != rank_ || (int)e >= S_) continue;
        hip_check(hipMemcpyAsync(hidden_ + H, relay_ + e * (size_t)H, sizeof(float) * H,
                                 hipMemcpyDeviceToDevice, st_), "selftest relay read");
        hip_check(hipMemcpyAsync(got.data(), hidden_ + H, sizeof(float) * H,
                                 hipMemcpyDeviceToHost, st_), "selftest D2H");
        hip_check(hipStreamSynchronize(st_), "selftest sync");
        int wrong = 0;
        for (int i = 0; i < H; ++i)
          if (got[i] != selftest_value((int)e + 64 * round, i)) ++wrong;
        if (wrong && bad.empty())
          bad = "rank " + std::to_string(rank_) + ": prefill relay from rank " +
                std::to_string(edges_[e].first) + " (edge " + std::to_string(e) + ", round " +
                std::to_string(round) + ") delivered " + std::to_string(wrong) + " wrong words";
      }
      ctl_.barrier();
    }
  }

  void selftest_pipeline() {
    const int H = cfg_.H;
    std::string bad;
    std::vector<float> pat(H + 4, 0.f);
    for (size_t e = 0; e < edges_.size(); ++e) {
      if (edges_[e].first != rank_) continue;
      for (int i = 0; i < H; ++i) pat[i] = selftest_value((int)e, i);
      const uint32_t tag = 0xC0DE0000u + (uint32_t)e;
      std::memcpy(&pat[H], &tag, 4);
      hip_check(hipMemcpyAsync(scratch_resid_, pat.data(), sizeof(float) * (H + 1),
                               hipMemcpyHostToDevice, st_), "selftest H2D");
      k_check(cake_hop_send(scratch_resid_, H, 1, hop_bf16_ ? 1 : 0, out_inbox_.at((int)e),
                            seq_ + 2 * e, st_), "selftest send");
      hip_check(hipStreamSynchronize(st_), "selftest sync");
    }
    for (size_t e = 0; e < edges_.size(); ++e) {
      if (edges_[e].second != rank_) continue;
      hip_check(hipMemsetAsync(scratch_resid_, 0, sizeof(float) * (H + 1), st_), "memset");
      k_check(cake_hop_recv(my_inbox_.at((int)e), H, 1, hop_bf16_ ? 1 : 0, scratch_resid_,
                            seq_ + 2 * e + 1, hop_err_, hop_timeout_, st_), "selftest recv");
      std::vector<float> got(H + 1);
      hip_check(hipMemcpyAsync(got.data(), scratch_resid_, sizeof(float) * (H + 1),
                               hipMemcpyDeviceToHost, st_), "selftest D2H");
      int herr = 0;
      hip_check(hipMemcpyAsync(&herr, hop_err_, sizeof(int), hipMemcpyDeviceToHost, st_), "err");
      hip_check(hipStreamSynchronize(st_), "selftest sync");
      const int src = edges_[e].first;
      uint32_t tag = 0;
      std::memcpy(&tag, &got[H], 4);
      int wrong = 0;
      for (int i = 0; i < H; ++i)
        if (got[i] != selftest_value((int)e, i)) ++wrong;
      if (herr) {
        bad = "rank " + std::to_string(rank_) + ": hop from rank " + std::to_string(src) +
              " (edge " + std::to_string(e) + ") timed out in the start-up self-test";
        hip_check(hipMemset(hop_err_, 0, sizeof(int)), "memset");
        break;
      }
      if (wrong || tag != 0xC0DE0000u + (uint32_t)e) {
        bad = "rank " + std::to_string(rank_) + ": hop from rank " + std::to_string(src) +
              " (edge " + std::to_string(e) + ") delivered " + std::to_string(wrong) +
              " wrong words in the start-up self-test";
        break;
      }
    }
    // the prefill relay buffers: every rank takes part whatever the hops found (the
    // rounds are lock-stepped through rank 0)
    selftest_relay(bad);
    if (bad.empty() && selftest_forced_fail())
      bad = "rank " + std::to_string(rank_) + ": failure forced by CAKE_IPC_SELFTEST_FAIL=1";
    // verdicts to rank 0, which fails every rank's start with the first bad edge named
    bad = ctl_.verdict(bad);
    if (!bad.empty()) throw Error("pipeline IPC self-test failed: " + bad);
  }

  // ---- tensor parallel (one process per GPU, every rank 1/W of every layer)
  void ar_sum() {
    k_check(cake_ar_sum(partial_, resid_, lc_.H, 1, ch_sum_.peers.data(), ch_sum_.inbox, ar_seq_,
                        ar_err_, tp_rank_, tp_, hop_timeout_, st_), "ar_sum");
  }

  // this rank's lm_head rows -> the global token on every rank (greedy: shard argmax key,
  // max over ranks; sampled: the full logits gathered, the single-GPU draw on each rank)
  void head_tp(const float* row, const Mode& m) {
    const Cfg& c = lc_;
    head_gemv(row);
    if (m.greedy) {
      k_check(cake_select_shard(logits_, c.V, voff_, hist_, hist_len_, m.last_n, m.penalty, 0.f,
                                0, slot_, st_), "select_shard");
      k_check(cake_ar_max_key(slot_, ch_key_.peers.data(), ch_key_.inbox, ar_seq_ + 2,
                              ar_err_ + 1, tp_rank_, tp_, hop_timeout_, st_), "ar_max_key");
    } else {
      const int V = cfg_.V;
      k_check(cake_ar_gather(logits_, voff_, c.V, full_logits_, V, ch_gat_.peers.data(),
                             ch_gat_.inbox, ar_seq_ + 4, ar_err_ + 2, tp_rank_, tp_,
                             hop_timeout_, st_), "ar_gather");
      if (m.penalty != 1.f)
        k_check(cake_repeat_penalty(full_logits_, hist_, hist_len_, m.last_n, m.penalty, st_),
                "penalty");
      const bool restrict = m.top_k > 0 || m.top_p > 0.f;
      if (restrict)
        k_check(cake_sample_threshold(full_logits_, V, m.temperature, m.top_k, m.top_p, thr_, st_),
                "sample_threshold");
      k_check(cake_gumbel_argmax(full_logits_, V, m.temperature, m.seed, hist_len_,
                                 restrict ? thr_ : nullptr, slot_, st_), "gumbel_argmax");
    }
    k_check(cake_finalize_token(slot_, tok_, hist_, hist_len_, pos_, S_, st_), "finalize");
  }

  // prefill: partial rows ppart_ [T, H] summed over the ranks into hidden_ — every rank
  // copies its rows into slot `rank` of every rank's slab (uncached device memory,
  // IPC-mapped), a barrier, then each sums the W slots; two slab banks, alternating, so
  // the next all-reduce never overwrites rows a slower rank still sums
  void dense_allreduce(int T) {
    const int R = slab_rows();
    const size_t SH = (size_t)R * cfg_.H;
    // rounds of R rows; the two banks alternate, so a peer's copies of round k + 1 never
    // land in the bank its sum of round k reads (each rank syncs its stream, sum
    // included, before the barrier that releases the next round's copies)
    for (int c0 = 0; c0 < T; c0 += R) {
      const int rows = std::min(R, T - c0);
      const size_t off = (size_t)c0 * cfg_.H, bytes = sizeof(float) * (size_t)rows * cfg_.H;
      const int bank = slab_bank_;
      slab_bank_ ^= 1;
      for (int p = 0; p < tp_; ++p) {
        float* base = p == tp_rank_ ? slab_ : static_cast<float*>(peer_slab_[p]);
        hip_check(hipMemcpyAsync(base + ((size_t)bank * tp_ + tp_rank_) * SH, ppart_ + off, bytes,
                                 hipMemcpyDeviceToDevice, st_), "slab copy");
      }
      hip_check(hipStreamSynchronize(st_), "sync");
      ctl_.barrier();  // host barrier over the control sockets
      k_check(cake_sum_slices(hidden_ + off, slab_ + (size_t)bank * tp_ * SH, tp_, (long long)SH,
                              (long long)rows * cfg_.H, 1, st_), "sum_slices");
    }
  }

  int slab_rows() const { return std::min(S_, kSlabRows); }

  static std::vector<int32_t> eos_of(const Json& m) {
    std::vector<int32_t> v;
    if (m.has("eos"))
      for (const auto& x : m.get("eos").items()) v.push_back((int32_t)x.as_int());
    return v;
  }

  // worker rank: run the generations rank 0 announces, in lock step
  void serve_tp() {
    for (;;) {
      const Json m = ctl_.recv(0);
      const std::string cmd = m.get("cmd").as_string();
      if (cmd == "exit") break;
      if (cmd == "generate") {
        std::vector<int32_t> prompt;
        for (const auto& x : m.get("prompt").items()) prompt.push_back((int32_t)x.as_int());
        CakeEngineSampling smp{};
        smp.temperature = (float)m.get("temperature").as_double();
        smp.top_k = (int32_t)m.get("top_k").as_int();
        smp.top_p = (float)m.get("top_p").as_double();
        smp.seed = std::strtoull(m.get("seed").as_string().c_str(), nullptr, 10);
        smp.repeat_penalty = (float)m.get("penalty").as_double();
        smp.repeat_last_n = (int32_t)m.get("last_n").as_int();
        const int max_new = (int)m.get("max_new").as_int();
        const std::vector<int32_t> eos = eos_of(m);
        run_generation(prompt.data(), (int)prompt.size(), max_new, smp, eos.data(),
                       (int)eos.size(), nullptr, nullptr, nullptr, 0, nullptr, false);
      } else if (cmd == "forced") {
        std::vector<int32_t> prompt, forced;
        for (const auto& x : m.get("prompt").items()) prompt.push_back((int32_t)x.as_int());
        for (const auto& x : m.get("forced").items()) forced.push_back((int32_t)x.as_int());
        forced_run(prompt.data(), (int)prompt.size(), forced.data(), (int)forced.size(), nullptr);
      } else if (cmd == "continue") {
        const std::vector<int32_t> eos = eos_of(m);
        const int L = read_i32(hist_len_);
        decode_tokens(L, (int)m.get("max_new").as_int(), eos.data(), (int)eos.size(), nullptr,
                      nullptr, nullptr, 0, false, nullptr);
      } else if (cmd == "sync") {
        reply_sync(ar_drain());
      } else {
        throw Error("unknown control message " + cmd);
      }
    }
  }

  // Start-up self-test of every tensor-parallel channel (before any graph exists): a
  // sum all-reduce of a rank-scaled pattern, the argmax-key max, the vocabulary gather
  // and the prefill slab all-reduce, each checked word for word; verdicts to rank 0.
  void selftest_tp() {
    const int H = cfg_.H, W = tp_;
    std::string bad;
    auto fail = [&](const std::string& what) {
      if (bad.empty()) bad = "tensor-parallel rank " + std::to_string(tp_rank_) + ": " + what;
    };
    std::vector<float> pat(H);
    for (int i = 0; i < H; ++i) pat[i] = (float)(tp_rank_ + 1) * (float)((i % 17) - 8);
    const float tri = (float)(W * (W + 1) / 2);
    // (1) decode sum channel
    hip_check(hipMemcpyAsync(partial_, pat.data(), sizeof(float) * H, hipMemcpyHostToDevice, st_),
              "selftest H2D");
    k_check(cake_ar_sum(partial_, scratch_resid_, H, 0, ch_sum_.peers.data(), ch_sum_.inbox,
                        ar_seq_, ar_err_, tp_rank_, tp_, hop_timeout_, st_), "selftest ar_sum");
    std::vector<float> got(H);
    hip_check(hipMemcpyAsync(got.data(), scratch_resid_, sizeof(float) * H, hipMemcpyDeviceToHost,
                             st_), "selftest D2H");
    hip_check(hipStreamSynchronize(st_), "sync");
    trace(rank(), "self-test: sum channel done");
    for (int i = 0; i < H; ++i)
      if (got[i] != tri * (float)((i % 17) - 8)) { fail("sum all-reduce delivered wrong words"); break; }
    // (2) argmax-key max channel
    const unsigned long long key = ((unsigned long long)(100 + tp_rank_) << 32) | (unsigned)tp_rank_;
    hip_check(hipMemcpyAsync(slot_, &key, sizeof(key), hipMemcpyHostToDevice, st_), "H2D");
    k_check(cake_ar_max_key(slot_, ch_key_.peers.data(), ch_key_.inbox, ar_seq_ + 2, ar_err_ + 1,
                            tp_rank_, tp_, hop_timeout_, st_), "selftest ar_max_key");
    unsigned long long mx = 0;
    hip_check(hipMemcpyAsync(&mx, slot_, sizeof(mx), hipMemcpyDeviceToHost, st_), "D2H");
    hip_check(hipStreamSynchronize(st_), "sync");
    if (mx != (((unsigned long long)(100 + W - 1) << 32) | (unsigned)(W - 1)))
      fail("argmax-key all-reduce returned a wrong key");
    trace(rank(), "self-test: key channel done");
    hip_check(hipMemsetAsync(slot_, 0, sizeof(unsigned long long), st_), "memset");
    // (3) vocabulary gather channel
    std::vector<float> shard(lc_.V);
    for (int j = 0; j < lc_.V; ++j) shard[j] = (float)(voff_ + j);
    hip_check(hipMemcpyAsync(logits_, shard.data(), sizeof(float) * lc_.V, hipMemcpyHostToDevice,
                             st_), "H2D");
    k_check(cake_ar_gather(logits_, voff_, lc_.V, full_logits_, cfg_.V, ch_gat_.peers.data(),
                           ch_gat_.inbox, ar_seq_ + 4, ar_err_ + 2, tp_rank_, tp_, hop_timeout_,
                           st_), "selftest ar_gather");
    std::vector<float> full(cfg_.V);
    hip_check(hipMemcpyAsync(full.data(), full_logits_, sizeof(float) * cfg_.V,
                             hipMemcpyDeviceToHost, st_), "D2H");
    hip_check(hipStreamSynchronize(st_), "sync");
    for (int j = 0; j < cfg_.V; ++j)
      if (full[j] != (float)j) { fail("vocabulary gather delivered wrong words"); break; }
    trace(rank(), "self-test: gather channel done");
    // (4) prefill slab all-reduce (one row)
    hip_check(hipMemcpyAsync(ppart_, pat.data(), sizeof(float) * H, hipMemcpyHostToDevice, st_),
              "H2D");
    hip_check(hipMemsetAsync(hidden_, 0, sizeof(float) * H, st_), "memset");
    dense_allreduce(1);
    hip_check(hipMemcpyAsync(got.data(), hidden_, sizeof(float) * H, hipMemcpyDeviceToHost, st_),
              "D2H");
    int errs[3] = {0, 0, 0};
    hip_check(hipMemcpyAsync(errs, ar_err_, sizeof(errs), hipMemcpyDeviceToHost, st_), "D2H");
    hip_check(hipStreamSynchronize(st_), "sync");
    for (int i = 0; i < H; ++i)
      if (got[i] != tri * (float)((i % 17) - 8)) { fail("prefill slab all-reduce delivered wrong words"); break; }
    // (5) two more rounds with new values (the banks alternate, so the second one
    // rewrites the bank of (4)): every rank has already read that bank's contents, so a
    // stale cached copy of a peer's slot fails here
    for (int round = 1; round <= 2; ++round) {  // collective: every rank runs both
      const float sc = -2.f - (float)round;
      for (int i = 0; i < H; ++i) pat[i] = sc * (float)(tp_rank_ + 1) * (float)((i % 13) - 6);
      hip_check(hipMemcpyAsync(ppart_, pat.data(), sizeof(float) * H, hipMemcpyHostToDevice,
                               st_), "H2D");
      hip_check(hipMemsetAsync(hidden_, 0, sizeof(float) * H, st_), "memset");
      dense_allreduce(1);
      hip_check(hipMemcpyAsync(got.data(), hidden_, sizeof(float) * H, hipMemcpyDeviceToHost,
                               st_), "D2H");
      hip_check(hipStreamSynchronize(st_), "sync");
      for (int i = 0; i < H; ++i)
        if (got[i] != sc * tri * (float)((i % 13) - 6)) {
          fail("prefill slab all-reduce (round " + std::to_string(round + 1) +
               ") delivered wrong words");
          break;
        }
    }
    hip_check(hipMemcpyAsync(errs, ar_err_, sizeof(errs), hipMemcpyDeviceToHost, st_), "D2H");
    hip_check(hipStreamSynchronize(st_), "sync");
    if (errs[0] | errs[1] | errs[2]) {
      fail("an all-reduce channel timed out");
      hip_check(hipMemset(ar_err_, 0, sizeof(errs)), "memset");
    }
    if (selftest_forced_fail()) fail("failure forced by CAKE_IPC_SELFTEST_FAIL=1");
    bad = ctl_.verdict(bad);
    if (!bad.empty()) throw Error("tensor-parallel IPC self-test failed: " + bad);
  }

  // channel inboxes (uncached, hop.hip granules) and the prefill slab, exchanged as IPC
  // handles through rank 0 (full mesh)
  void connect_tp(const std::string& addr, double timeout_s) {
    auto alloc = [&](size_t words) {
      void* p = nullptr;
      k_check(cake_hop_alloc(words * 8, &p), "hop_alloc");
      tp_owned_.push_back(p);
      return p;
    };
    ch_sum_.inbox = alloc((size_t)cake_ar_inbox_words(tp_, cfg_.H));
    ch_key_.inbox = alloc((size_t)cake_ar_inbox_words(tp_, 2));
    ch_gat_.inbox = alloc(2 * (size_t)cfg_.V);
    const size_t slab_bytes = sizeof(float) * 2 * (size_t)tp_ * slab_rows() * cfg_.H;
    void* sp = nullptr;
    hip_check(hipExtMallocWithFlags(&sp, slab_bytes, hipDeviceMallocUncached), "slab alloc");
    tp_owned_.push_back(sp);
    slab_ = static_cast<float*>(sp);
    trace(rank(), "tensor-parallel inboxes + slab allocated (" +
                      std::to_string(slab_bytes >> 20) + " MiB slab)");
    void* mine[4] = {ch_sum_.inbox, ch_key_.inbox, ch_gat_.inbox, slab_};
    Json me = Json::array();
    for (void* p : mine) me.push(Json::string(ipc_export(p)));
    ctl_.open(addr, tp_rank_, tp_, me, timeout_s, "bad TP rank hello");
    trace(rank(), "tensor-parallel handle table exchanged");
    ArChan* chans[3] = {&ch_sum_, &ch_key_, &ch_gat_};
    for (auto* ch : chans) ch->peers.assign(tp_, nullptr);
    peer_slab_.assign(tp_, nullptr);
    for (int r = 0; r < tp_; ++r) {
      if (r == tp_rank_) continue;
      for (int k = 0; k < 4; ++k) {
        void* p = ipc_import(ctl_.table()[r].at(k).as_string(), "IpcOpen");
        tp_mapped_.push_back(p);
        if (k < 3) chans[k]->peers[r] = p;
        else peer_slab_[r] = p;
      }
    }
  }

  void drop_graphs() {
    for (auto e : execs_) (void)hipGraphExecDestroy(e);
    for (auto g : graphs_) (void)hipGraphDestroy(g);
    execs_.clear();
    graphs_.clear();
    have_graphs_ = false;
  }

  // one graph per attention split cap (DeviceDecoder.capture position buckets)
  void ensure_graphs(const Mode& m) {
    if (have_graphs_ && graph_mode_ == m) return;
    trace(rank(), "capturing decode graphs");
    drop_graphs();
    if (!head_) {  // pipeline worker: its layers once, eagerly, at position 0 (the row is
                   // rewritten by every prefill), so no kernel's first launch is captured
      hip_check(hipMemsetAsync(resid_, 0, sizeof(float) * (cfg_.H + 1), st_), "memset");
      step_layers();
      hip_check(hipStreamSynchronize(st_), "sync");
    }
    if (world_ == 1) warm_step(m);
    capture_buckets(m);
  }

  // warm every kernel once outside capture on the live state, then restore it (the
  // K/V row this writes is the next step's, which that step rewrites)
  void warm_step(const Mode& m) {
    hip_check(hipMemcpyAsync(scratch_i32_, tok_, sizeof(int), hipMemcpyDeviceToDevice, st_), "snap");
    hip_check(hipMemcpyAsync(scratch_i32_ + 1, pos_, sizeof(int), hipMemcpyDeviceToDevice, st_), "snap");
    hip_check(hipMemcpyAsync(scratch_i32_ + 2, hist_len_, sizeof(int), hipMemcpyDeviceToDevice, st_), "snap");
    hip_check(hipMemcpyAsync(scratch_resid_, resid_, sizeof(float) * cfg_.H, hipMemcpyDeviceToDevice, st_), "snap");
    step_body(m);
    hip_check(hipMemcpyAsync(tok_, scratch_i32_, sizeof(int), hipMemcpyDeviceToDevice, st_), "restore");
    hip_check(hipMemcpyAsync(pos_, scratch_i32_ + 1, sizeof(int), hipMemcpyDeviceToDevice, st_), "restore");
    hip_check(hipMemcpyAsync(hist_len_, scratch_i32_ + 2, sizeof(int), hipMemcpyDeviceToDevice, st_), "restore");
    hip_check(hipMemcpyAsync(resid_, scratch_resid_, sizeof(float) * cfg_.H, hipMemcpyDeviceToDevice, st_), "restore");
    hip_check(hipMemsetAsync(slot_, 0, sizeof(unsigned long long), st_), "slot");
    hip_check(hipStreamSynchronize(st_), "sync");
  }

  void capture_buckets(const Mode& m) {
    // caps: 8 / 16 / 32 / 64 (clamped to the max_seq grid) up to the first covering
    // every live length (ops.hip.attn_split_caps)
    const int full = cake_attn_max_split(S_);
    int need = 1;
    for (int t = 1; t <= S_; ++t) need = std::max(need, cake_attn_splits(t));
    std::vector<int> caps;
    for (int cap : {8, 16, 32, 64}) {
      const int cc = std::min(cap, full);
      if (std::find(caps.begin(), caps.end(), cc) == caps.end()) caps.push_back(cc);
      if (cap >= need) break;
    }
    // cap 1: the one-split lengths with attention + o_proj fused (attn_oproj.hip), or the
    // short lengths on the head-parallel attention
    if (ao_ok_ || heads_max_ > 0) caps.push_back(1);
    std::sort(caps.begin(), caps.end());
    try {
      for (int cap : caps) {
        k_check(cake_attn_set_split_cap(cap == 1 ? full : cap), "attn_set_split_cap");
        hipGraph_t g = nullptr;
        short_step_ = cap == 1;
        hip_check(hipStreamBeginCapture(st_, hipStreamCaptureModeGlobal), "BeginCapture");
        try {
          for (int i = 0; i < k_; ++i) step_body(m);
        } catch (...) {
          short_step_ = false;
          (void)hipStreamEndCapture(st_, &g);
          if (g) (void)hipGraphDestroy(g);
          throw;
        }
        short_step_ = false;
        hip_check(hipStreamEndCapture(st_, &g), "EndCapture");
        graphs_.push_back(g);
        hipGraphExec_t e = nullptr;
        hip_check(hipGraphInstantiate(&e, g, nullptr, nullptr, 0), "GraphInstantiate");
        execs_.push_back(e);
      }
    } catch (...) {
      (void)cake_attn_set_split_cap(0);
      drop_graphs();
      throw;
    }
    k_check(cake_attn_set_split_cap(0), "attn_set_split_cap");
    bucket_of_.assign(S_ + 1, (int32_t)caps.size() - 1);
    for (int t = 0; t <= S_; ++t) {
      const int nd = cake_attn_splits(t);
      const bool sh = short_len(t);
      for (size_t i = 0; i < caps.size(); ++i)
        if ((caps[i] == 1) == sh && caps[i] >= nd) { bucket_of_[t] = (int32_t)i; break; }
    }
    graph_mode_ = m;
    have_graphs_ = true;
  }
};

void put_err(char* err, int errlen, const std::string& msg) {
  if (err && errlen > 0) {
    std::snprintf(err, (size_t)errlen, "%s", msg.c_str());
  }
}

}  // namespace
}  // namespace cake

using cake::Llama;

CAKE_API void* cake_engine_open(const char* model_dir, const CakeEngineOpts* opts, char* err,
                                int32_t errlen) {
  try {
    if (!model_dir || !opts) throw cake::Error("null argument");
    return new Llama(model_dir, *opts);
  } catch (const std::exception& e) {
    cake::put_err(err, errlen, e.what());
    return nullptr;
  }
}

CAKE_API void* cake_engine_open_pp(const char* model_dir, const CakeEngineOpts* opts,
                                   const CakePipeOpts* pipe, char* err, int32_t errlen) {
  try {
    if (!model_dir || !opts || !pipe) throw cake::Error("null argument");
    return new Llama(model_dir, *opts, pipe);
  } catch (const std::exception& e) {
    cake::put_err(err, errlen, e.what());
    return nullptr;
  }
}

CAKE_API void* cake_engine_open_remote(const char* model_dir, const CakeEngineOpts* opts,
                                       const CakeRemoteOpts* remote, char* err, int32_t errlen) {
  try {
    if (!model_dir || !opts || !remote) throw cake::Error("null argument");
    return new Llama(model_dir, *opts, nullptr, nullptr, nullptr, remote);
  } catch (const std::exception& e) {
    cake::put_err(err, errlen, e.what());
    return nullptr;
  }
}

CAKE_API void* cake_engine_open_layers(const char* model_dir, const CakeEngineOpts* opts,
                                       const int32_t* layers, int32_t n_layers, char* err,
                                       int32_t errlen) {
  try {
    if (!model_dir || !opts || !layers || n_layers <= 0) throw cake::Error("bad arguments");
    const std::vector<int> ls(layers, layers + n_layers);
    return new Llama(model_dir, *opts, nullptr, &ls);
  } catch (const std::exception& e) {
    cake::put_err(err, errlen, e.what());
    return nullptr;
  }
}

CAKE_API int32_t cake_engine_forward(void* h, uint64_t session, const int32_t* layers,
                                     int32_t n_layers, int32_t pos0, float* hidden, int32_t T,
                                     char* err, int32_t errlen) {
  try {
    if (!h || !layers || !hidden) throw cake::Error("null argument");
    static_cast<Llama*>(h)->forward_host(session, std::vector<int>(layers, layers + n_layers),
                                         pos0, hidden, T);
    return 0;
  } catch (const std::exception& e) {
    cake::put_err(err, errlen, e.what());
    return 1;
  }
}

CAKE_API void cake_engine_drop_session(void* h, uint64_t session) {
  try {
    if (h) static_cast<Llama*>(h)->drop_session(session);
  } catch (const std::exception&) {
  }
}

CAKE_API void* cake_engine_open_tp(const char* model_dir, const CakeEngineOpts* opts,
                                   const CakeTPOpts* tp, char* err, int32_t errlen) {
  try {
    if (!model_dir || !opts || !tp) throw cake::Error("null argument");
    if (CAKE_WEIGHT_FMT_OF(opts->weight_fmt) != 0) throw cake::Error(cake::kNoFp8TP);
    if (CAKE_PREFILL_FMT_OF(opts->weight_fmt) != 0) throw cake::Error(cake::kNoPrefillTP);
    if (opts->head_fmt != 0) throw cake::Error(cake::kNoQHeadTP);
    if (opts->kv_fmt != 0) throw cake::Error(cake::kNoKvTP);
    return new Llama(model_dir, *opts, nullptr, nullptr, tp);
  } catch (const std::exception& e) {
    cake::put_err(err, errlen, e.what());
    return nullptr;
  }
}

CAKE_API int32_t cake_engine_serve(void* h, char* err, int32_t errlen) {
  try {
    if (!h) throw cake::Error("null engine");
    static_cast<Llama*>(h)->serve();
    return 0;
  } catch (const std::exception& e) {
    cake::put_err(err, errlen, e.what());
    return 1;
  }
}

CAKE_API int32_t cake_engine_rank_info(void* h, int32_t* o) {
  if (!h || !o) return (int32_t)hipErrorInvalidValue;
  const Llama* m = static_cast<Llama*>(h);
  const auto lr = m->layer_range();
  o[0] = m->rank();
  o[1] = m->world();
  o[2] = lr.first;
  o[3] = lr.second;
  return 0;
}

CAKE_API int32_t cake_engine_info(void* h, int32_t* o) {
  if (!h || !o) return (int32_t)hipErrorInvalidValue;
  const Llama* m = static_cast<Llama*>(h);
  const auto& c = m->cfg();
  const int32_t v[8] = {c.V, c.H, c.L, c.nh, c.nkv, c.hd, c.I, m->max_seq()};
  std::memcpy(o, v, sizeof(v));
  return 0;
}

CAKE_API int64_t cake_engine_kv_bytes(void* h) {
  return h ? static_cast<Llama*>(h)->kv_bytes() : 0;
}

CAKE_API int64_t cake_engine_weight_bytes(void* h) {
  return h ? static_cast<Llama*>(h)->weight_bytes() : 0;
}

CAKE_API int64_t cake_engine_packed_bytes(void* h) {
  return h ? static_cast<Llama*>(h)->packed_bytes() : 0;
}

CAKE_API int32_t cake_engine_eos(void* h, int32_t* out, int32_t cap) {
  if (!h) return 0;
  const auto& e = static_cast<Llama*>(h)->cfg().eos;
  for (int32_t i = 0; i < cap && i < (int32_t)e.size(); ++i) out[i] = e[i];
  return (int32_t)e.size();
}

CAKE_API int32_t cake_engine_generate(void* h, const int32_t* prompt, int32_t n_prompt,
                                      int32_t max_new, const CakeEngineSampling* sampling,
                                      const int32_t* eos, int32_t n_eos,
                                      cake_engine_token_cb cb, void* ctx, int32_t* out,
                                      int32_t out_cap, CakeEngineStats* stats, char* err,
                                      int32_t errlen) {
  try {
    if (!h || !prompt || !sampling || (!out && max_new > 0)) throw cake::Error("null argument");
    static_cast<Llama*>(h)->generate(prompt, n_prompt, max_new, *sampling, eos, n_eos, cb, ctx,
                                     out, out_cap, stats);
    return 0;
  } catch (const std::exception& e) {
    cake::put_err(err, errlen, e.what());
    return 1;
  }
}

CAKE_API int32_t cake_engine_generate_batch(void* h, const int32_t* tokens, const int32_t* offsets,
                                            int32_t n_seq, int32_t max_new,
                                            const CakeEngineSampling* sampling, const int32_t* eos,
                                            int32_t n_eos, int32_t* out, int32_t* out_len,
                                            CakeEngineStats* seq_stats, CakeEngineStats* stats,
                                            float* logits_out, char* err, int32_t errlen) {
  try {
    if (!h || !tokens || !offsets || !sampling || !out_len || (!out && max_new > 0) ||
        (!eos && n_eos > 0))
      throw cake::Error("null argument");
    static_cast<Llama*>(h)->generate_batch(tokens, offsets, n_seq, max_new, *sampling, eos, n_eos,
                                           out, out_len, seq_stats, stats, logits_out);
    return 0;
  } catch (const std::exception& e) {
    cake::put_err(err, errlen, e.what());
    return 1;
  }
}

CAKE_API int32_t cake_engine_continue(void* h, int32_t max_new, const int32_t* eos, int32_t n_eos,
                                      cake_engine_token_cb cb, void* ctx, int32_t* out,
                                      int32_t out_cap, CakeEngineStats* stats, char* err,
                                      int32_t errlen) {
  try {
    if (!h || (!out && max_new > 0)) throw cake::Error("null argument");
    static_cast<Llama*>(h)->continue_gen(max_new, eos, n_eos, cb, ctx, out, out_cap, stats);
    return 0;
  } catch (const std::exception& e) {
    cake::put_err(err, errlen, e.what());
    return 1;
  }
}

CAKE_API int32_t cake_engine_forced_logits(void* h, const int32_t* prompt, int32_t n_prompt,
                                           const int32_t* forced, int32_t n_forced, float* out,
                                           char* err, int32_t errlen) {
  try {
    if (!h || !prompt || (!forced && n_forced > 0) || !out) throw cake::Error("null argument");
    static_cast<Llama*>(h)->forced_logits(prompt, n_prompt, forced, n_forced, out);
    return 0;
  } catch (const std::exception& e) {
    cake::put_err(err, errlen, e.what());
    return 1;
  }
}

CAKE_API int32_t cake_engine_score(void* h, const int32_t* tokens, int32_t n, int32_t vchunk,
                                   float* lse, float* tgt, int32_t* top, float* topv, char* err,
                                   int32_t errlen) {
  try {
    if (!h || !tokens || !lse || !tgt || !top || !topv) throw cake::Error("null argument");
    static_cast<Llama*>(h)->score(tokens, n, vchunk, lse, tgt, top, topv);
    return 0;
  } catch (const std::exception& e) {
    cake::put_err(err, errlen, e.what());
    return 1;
  }
}

CAKE_API int32_t cake_engine_set_logprobs(void* h, int32_t top_k, char* err, int32_t errlen) {
  try {
    if (!h) throw cake::Error("null engine");
    static_cast<Llama*>(h)->set_logprobs(top_k);
    return 0;
  } catch (const std::exception& e) {
    cake::put_err(err, errlen, e.what());
    return 1;
  }
}

CAKE_API int32_t cake_engine_set_logit_controls(void* h, const CakeLogitControls* c, char* err,
                                                int32_t errlen) {
  try {
    if (!h) throw cake::Error("null engine");
    static_cast<Llama*>(h)->set_logit_controls(c);
    return 0;
  } catch (const std::exception& e) {
    cake::put_err(err, errlen, e.what());
    return 1;
  }
}

CAKE_API int32_t cake_engine_logprobs(void* h, int32_t first, int32_t count, int32_t* ids,
                                      float* logit, float* lse, int32_t* top_ids,
                                      float* top_logits, char* err, int32_t errlen) {
  try {
    if (!h || ((!ids || !logit || !lse || !top_ids || !top_logits) && count > 0))
      throw cake::Error("null argument");
    static_cast<Llama*>(h)->logprobs(first, count, ids, logit, lse, top_ids, top_logits);
    return 0;
  } catch (const std::exception& e) {
    cake::put_err(err, errlen, e.what());
    return 1;
  }
}

// "rank:first-last,..." runs of the token's walk (placement check), n = bytes written
CAKE_API int32_t cake_engine_walk(void* h, char* out, int32_t cap) {
  if (!h || !out || cap <= 0) return 0;
  const std::string s = static_cast<Llama*>(h)->walk_str();
  const int32_t n = (int32_t)std::min<size_t>(s.size(), (size_t)cap - 1);
  std::memcpy(out, s.data(), (size_t)n);
  out[n] = 0;
  return n;
}

CAKE_API int32_t cake_engine_prefill_logits(void* h, const int32_t* prompt, int32_t n_prompt,
                                            float* out, char* err, int32_t errlen) {
  try {
    if (!h || !prompt || !out) throw cake::Error("null argument");
    static_cast<Llama*>(h)->prefill_logits(prompt, n_prompt, out);
    return 0;
  } catch (const std::exception& e) {
    cake::put_err(err, errlen, e.what());
    return 1;
  }
}

CAKE_API void cake_engine_close(void* h) { delete static_cast<Llama*>(h); }
