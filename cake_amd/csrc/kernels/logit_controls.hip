// Per-request logit controls on the f32 row x[V] token selection sees: OpenAI's presence /
// frequency penalties over the tokens generated so far, logit_bias, and the min_p cut.  One
// launch per decode step, between the repeat penalty and the argmax / draw:
//   c[v] = occurrences of v in generated = hist[gen0, hist_len)
//   c[v] > 0:      x[v] = x[v] - (presence + frequency * float(c[v]))   each op rounded to f32
//   (id, b) listed: x[id] = x[id] + b                                    after the penalty
//   min_p on:      cut = max_v x[v] + d, d = float32(T ln min_p) from the host; the sampling
//                  set is ordered(x[v]) >= min(ordered(cut), ordered(max)) (the second term only
//                  matters for a maximum of -0.0 with d = 0, whose sum is +0.0)
// ops/reference.py::logit_controls_ref is the numpy float32 oracle, bit for bit.
//
// Counts are a resident table cnt[V] (u32) that always equals the histogram of
// hist[gen0, counted): every launch adds the entries hist[counted, hist_len), normally one, and
// the last workgroup publishes counted = hist_len.  A step run twice on one history length (the
// engine's warm step) therefore counts nothing twice.  hist_len < counted adds nothing and leaves
// counted alone; the caller clears the table and sets counted = gen0 when a generation starts.
//
// Owner computes: the row is spread over G <= 64 workgroups of 256 threads in contiguous slices
// of whole 2048-column pieces (logprob.hip's plan), and every vocabulary id belongs to one
// thread, which adds the new occurrences of its ids to its own cnt entries (plain integer
// stores: deterministic, no atomics), applies penalty then bias to its own elements and folds
// the adjusted values into its running maximum.  An id that is counted and biased thus gets
// both in order whichever workgroup owns it, and the row is read once.  cnt and x are written
// back only where they changed.  The bias list (<= 300 distinct ids) is scattered per piece into
// an LDS table of list positions, so an element costs one LDS read, not a search.
//
// Hand-off: each workgroup stores its maximum key to state[4 + g], drains, barrier, thread 0
// issues an agent-scope release fence and draws a ticket (one integer atomic per workgroup on a
// shared word: they serialise, see argmax_grid in sampling.hip).  The workgroup that draws
// G - 1 acquires, folds the G keys in one wave, writes counted, the row maximum key and the cut
// key, and re-arms the ticket, so launches need no host reset between them and replay in a graph.
//
// Device blocks (32-bit words; sizes in cake_kernels.h):
//   params[kLcParamWords]: 0 presence | 1 frequency | 2 d | 3 gen0 | 4 n_bias | 5 min_p on |
//                          6, 7 zero | 8..307 bias ids | 308..607 bias values
//   state[kLcStateWords]:  0 ticket | 1 counted | 2 cut key (0: no restriction) | 3 key of the
//                          adjusted row's maximum | 4..67 per-workgroup maxima
#include "common.h"
#include "reduce64.h"

namespace cake {

constexpr int kLcThreads = 256;
constexpr int kLcNV = 2;                            // 16-byte loads per thread and piece
constexpr int kLcPiece = kLcThreads * kLcNV * 4;    // 2048 columns
constexpr int kLcMaxBlocks = 64;                    // one wave folds the maxima
constexpr unsigned short kLcNoBias = 0xffffu;
// kLcMaxBias = 300, kLcParamWords = 608, kLcStateWords = 68: cake_kernels.h

struct LcCtx {
  const int32_t* hist;
  int new_lo, new_hi;     // history entries to add to the table
  float presence, frequency;
  bool penal, biased;
  const float* bias_val;
  const unsigned short* bslot;  // LDS: list position of piece column c at [c], or kLcNoBias
};

// one owned element: vocabulary id `id`, piece column `col`; returns the adjusted value
__device__ __forceinline__ float lc_element(const LcCtx& k, float x, unsigned int& c,
                                            unsigned int id, int col, bool& x_dirty,
                                            bool& c_dirty) {
  // every product, sum and difference rounded on its own (the oracle's arithmetic), so no
  // fused multiply-add here (__fmul_rn under __fadd_rn still contracts: plain operators in
  // this scope do not)
#pragma clang fp contract(off)
  for (int i = k.new_lo; i < k.new_hi; ++i)
    if ((unsigned int)k.hist[i] == id) { ++c; c_dirty = true; }
  if (k.penal && c > 0u) {
    const float fc = k.frequency * (float)c;
    const float pen = k.presence + fc;
    x = x - pen;
    x_dirty = true;
  }
  if (k.biased) {
    const unsigned short e = k.bslot[col];
    if (e != kLcNoBias) { x = x + k.bias_val[e]; x_dirty = true; }
  }
  return x;
}

__global__ __launch_bounds__(kLcThreads) void logit_controls_kernel(
    float* __restrict__ logits, int V, int per, const int32_t* __restrict__ hist,
    const int32_t* __restrict__ hist_len, unsigned int* __restrict__ cnt,
    const unsigned int* __restrict__ params, unsigned int* state) {
  __shared__ unsigned short bslot[kLcPiece];
  __shared__ unsigned int red[kLcThreads / 64 + 1];
  const int tid = threadIdx.x;
  const int G = gridDim.x, g = blockIdx.x;
  const int c_lo = g * per, len = min(V - c_lo, per);  // c_lo < V: the grid is ceil(V / per)
  const int n_bias = min(max((int)params[4], 0), kLcMaxBias);
  const int hl = *hist_len;
  const int counted = (int)__hip_atomic_load(state + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const int32_t* bias_id = reinterpret_cast<const int32_t*>(params + 8);

  LcCtx k;
  k.hist = hist;
  k.new_lo = max(counted, 0);
  k.new_hi = hl;  // hl <= counted: an empty range
  k.presence = __uint_as_float(params[0]);
  k.frequency = __uint_as_float(params[1]);
  k.penal = k.presence != 0.f || k.frequency != 0.f;
  k.biased = n_bias > 0;
  k.bias_val = reinterpret_cast<const float*>(params + 8 + kLcMaxBias);
  k.bslot = bslot;

  unsigned int best = 0u;  // below the key of every float
  for (int o = 0; o < len; o += kLcPiece) {
    float* const src = logits + c_lo + o;
    unsigned int* const csrc = cnt + c_lo + o;
    const int n = min(len - o, kLcPiece);
    const unsigned int g0 = (unsigned int)(c_lo + o);
    if (k.biased) {  // uniform
      __syncthreads();  // the previous piece's reads are done
      for (int i = tid; i < kLcPiece; i += kLcThreads) bslot[i] = kLcNoBias;
      __syncthreads();
      for (int e = tid; e < n_bias; e += kLcThreads) {
        const unsigned int d = (unsigned int)bias_id[e] - g0;
        if (d < (unsigned int)n) bslot[d] = (unsigned short)e;  // ids are distinct
      }
      __syncthreads();
    }
    // columns [0, lead) and [lead + 4 nvec, n) one by one, the 16-byte aligned middle of the
    // row 16 bytes each (score.hip's scheme); the counts take 16-byte accesses where the same
    // columns are aligned in the table
    const int lead = min(n, (int)(((16u - (unsigned int)((uintptr_t)src & 15u)) & 15u) >> 2));
    const int nvec = (n - lead) >> 2;
    const int ntail = n - lead - 4 * nvec;
    const bool cvec = (((uintptr_t)(csrc + lead)) & 15u) == 0u;
    int cs = -1;  // lead + ntail <= 6
    if (tid < lead) cs = tid;
    else if (tid < lead + ntail) cs = lead + 4 * nvec + (tid - lead);
    if (cs >= 0) {
      unsigned int c = csrc[cs];
      bool xd = false, cd = false;
      const float x = lc_element(k, src[cs], c, g0 + (unsigned int)cs, cs, xd, cd);
      if (cd) csrc[cs] = c;
      if (xd) src[cs] = x;
      best = max(best, score_ordered(x));
    }
#pragma unroll
    for (int j = 0; j < kLcNV; ++j) {
      const int v = j * kLcThreads + tid;
      if (v < nvec) {
        const int col = lead + 4 * v;
        float4 r = *reinterpret_cast<const float4*>(src + col);
        uint4 c;
        if (cvec) {
          c = *reinterpret_cast<const uint4*>(csrc + col);
        } else {
          c.x = csrc[col];
          c.y = csrc[col + 1];
          c.z = csrc[col + 2];
          c.w = csrc[col + 3];
        }
        bool xd = false, cd = false;
        const unsigned int gi = g0 + (unsigned int)col;
        r.x = lc_element(k, r.x, c.x, gi, col, xd, cd);
        r.y = lc_element(k, r.y, c.y, gi + 1, col + 1, xd, cd);
        r.z = lc_element(k, r.z, c.z, gi + 2, col + 2, xd, cd);
        r.w = lc_element(k, r.w, c.w, gi + 3, col + 3, xd, cd);
        if (cd) {
          if (cvec) {
            *reinterpret_cast<uint4*>(csrc + col) = c;
          } else {
            csrc[col] = c.x;
            csrc[col + 1] = c.y;
            csrc[col + 2] = c.z;
            csrc[col + 3] = c.w;
          }
        }
        if (xd) *reinterpret_cast<float4*>(src + col) = r;
        best = max(best, max(max(score_ordered(r.x), score_ordered(r.y)),
                             max(score_ordered(r.z), score_ordered(r.w))));
      }
    }
  }

  // the workgroup's maximum key -> state[4 + g]
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) best = max(best, (unsigned int)__shfl_xor((int)best, off, 64));
  if ((tid & 63) == 0) red[tid >> 6] = best;
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int w = 1; w < kLcThreads / 64; ++w) best = max(best, red[w]);
    state[4 + g] = best;
  }
  // publish; the last workgroup folds all G maxima (see the header)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned int drawn =
        __hip_atomic_fetch_add(state, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const bool last = drawn == (unsigned int)(G - 1);
    if (last) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __hip_atomic_store(state, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // re-arm
    }
    red[kLcThreads / 64] = last ? 1u : 0u;
  }
  __syncthreads();
  if (red[kLcThreads / 64] == 0u || tid >= 64) return;

  unsigned int m = tid < G ? __builtin_nontemporal_load(state + 4 + tid) : 0u;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) m = max(m, (unsigned int)__shfl_xor((int)m, off, 64));
  if (tid == 0) {
    unsigned int cut = 0u;
    if (params[5] != 0u) {
      const float c = __fadd_rn(score_unordered(m), __uint_as_float(params[2]));
      cut = min(score_ordered(c), m);
    }
    if (hl > counted) state[1] = (unsigned int)hl;
    state[2] = cut;
    state[3] = m;
  }
}

__global__ void lc_merge_thr_kernel(unsigned int* __restrict__ thr,
                                    const unsigned int* __restrict__ cut) {
  const unsigned int a = *thr, b = *cut;
  *thr = a > b ? a : b;
}

}  // namespace cake

using namespace cake;

// One pass of the controls in `params` over logits[V] (see the header).  cnt: V words, the count
// table; state: kLcStateWords words, zeroed once at allocation (word 1, counted, is the
// caller's to set with the table).  hist / hist_len: the device history.  max_blocks 0: the
// default grid.  Every id of hist[counted, *hist_len) must lie in [0, V) to be counted; others
// are ignored.
CAKE_API int cake_logit_controls(float* logits, int V, const int32_t* hist,
                                 const int32_t* hist_len, unsigned int* cnt, const void* params,
                                 unsigned int* state, int max_blocks, hipStream_t st) {
  if (!logits || !hist || !hist_len || !cnt || !params || !state || V < 1 || max_blocks < 0 ||
      ((uintptr_t)logits & 3u) || ((uintptr_t)cnt & 3u) || ((uintptr_t)params & 3u) ||
      ((uintptr_t)state & 3u))
    return (int)hipErrorInvalidValue;
  const int pieces = (V + kLcPiece - 1) / kLcPiece;
  const int cap = max_blocks > 0 && max_blocks < kLcMaxBlocks ? max_blocks : kLcMaxBlocks;
  const int g0 = pieces < cap ? pieces : cap;
  const long long p = (long long)((pieces + g0 - 1) / g0) * kLcPiece;
  const int per = (int)(p > 0x7fffffffLL ? 0x7fffffffLL : p);
  const int grid = (int)((V + p - 1) / p);
  hipLaunchKernelGGL(logit_controls_kernel, dim3(grid), dim3(kLcThreads), 0, st, logits, V, per,
                     hist, hist_len, cnt, static_cast<const unsigned int*>(params), state);
  return (int)hipGetLastError();
}

// *thr = max(*thr, *cut): the min_p cut key merged into the top-k / top-p threshold key
CAKE_API int cake_logit_controls_merge_thr(unsigned int* thr, const unsigned int* cut,
                                           hipStream_t st) {
  if (!thr || !cut) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(lc_merge_thr_kernel, dim3(1), dim3(1), 0, st, thr, cut);
  return (int)hipGetLastError();
}
