// Log-probs of a generated token: over the f32 row x[V] that token selection saw, one launch
// writes a 192-byte record with the chosen token's logit, the row's log-sum-exp and the K
// largest logits (K <= 20) with their ids.  The host forms logprob = logit - lse in f64.
//
// Record, 48 words at rec + idx * 192 with idx = *hist_len - 1 (the history slot the token
// was just written to); an idx outside [0, max_rec) writes nothing:
//   0 token id | 1 logit bits | 2 lse bits (f32) | 3 K | 4..23 top ids | 24..43 top logit
//   bits | 44..47 zero.  Top entries past min(K, V): id -1, logit -inf.
// Order: descending logit, the lower id first at ties: the (ordered(x) << 32) | ~id key of
// head-select and score.hip (reduce64.h).  Keys of distinct ids are distinct, so "the largest
// key below the previous one" walks the order one entry per round.
//
// The row is spread over G <= 64 workgroups of 256 threads; each takes a contiguous slice of
// whole 2048-column pieces.  One piece stays in registers as keys (the logit is recovered from
// the key bit for bit), so with the default grid (one piece per slice at V <= 131072) the row
// is read once: slice maximum, S = sum exp(x - max) with score.hip's arithmetic (v_exp_f32
// terms, f64 additions), then K rounds for the slice's own top K.  A slice must keep K
// candidates, not one: the row's K largest logits may all lie in it.  A longer slice
// (max_blocks below the default) loops over pieces with score.hip's running merge and re-reads
// them in every round.
//
// Hand-off: each workgroup writes its partial {S, max, K keys} to ws with plain stores, every
// wave drains (s_waitcnt vmcnt(0)), barrier, then thread 0 issues an agent-scope release
// fence, drains again and adds to the ticket (relaxed, agent scope).  The workgroup that draws
// G - 1 issues an agent-scope acquire fence before any of its threads read ws (the barrier
// after it holds the other waves), and reads ws with vector loads.  This is the plain-store
// release / acquire form of the in-launch split-K recipe, as gn_nhwc_stats_kernel uses it.
// The last workgroup re-arms the ticket (the caller zeroes it once, at allocation), so
// launches need no host state between them and replay inside a graph.
//
// The merge is by slice index, never by arrival: lane g of one wave scales slice g's sum to
// the row maximum and the lanes are added by the fixed butterfly of wave_sum_f64, so the lse
// bits are the same whichever workgroup finishes last.  lse = max + log(S) in f64, stored f32;
// -inf if every logit is -inf.
#include "common.h"
#include "reduce64.h"

namespace cake {

constexpr int kLpThreads = 256;
constexpr int kLpNV = 2;                                // 16-byte loads per thread and piece
constexpr int kLpPiece = kLpThreads * kLpNV * 4;        // 2048 columns
constexpr int kLpKeys = kLpNV * 4 + 1;                  // + this thread's scalar column
constexpr int kLpMaxBlocks = 64;                        // one wave merges the partials
constexpr int kLpSlot = 24;                             // u64 words per partial: S, max, 20 keys
// kLpMaxK = 20, kLpRecWords = 48: cake_kernels.h

// keys of piece columns [0, n) at src (vocabulary id g0 + column); empty slots are 0, which
// is below every real key.  Columns [0, lead) and [lead + 4 nvec, n) are read one by one, the
// 16-byte aligned middle 16 bytes each (score.hip's scheme).
__device__ __forceinline__ void lp_load(const float* __restrict__ src, int n, unsigned int g0,
                                        int tid, unsigned long long (&kk)[kLpKeys]) {
  const int lead = min(n, (int)(((16u - (unsigned int)((uintptr_t)src & 15u)) & 15u) >> 2));
  const int nvec = (n - lead) >> 2;
  const int ntail = n - lead - 4 * nvec;
  int cs = -1;  // lead + ntail <= 6
  if (tid < lead) cs = tid;
  else if (tid < lead + ntail) cs = lead + 4 * nvec + (tid - lead);
  kk[kLpKeys - 1] = cs >= 0 ? score_key(src[cs], g0 + (unsigned int)cs) : 0ull;
#pragma unroll
  for (int j = 0; j < kLpNV; ++j) {
    const int c = j * kLpThreads + tid;
    if (c < nvec) {
      const float4 r = *reinterpret_cast<const float4*>(src + lead + 4 * c);
      const unsigned int gi = g0 + (unsigned int)(lead + 4 * c);
      kk[4 * j + 0] = score_key(r.x, gi);
      kk[4 * j + 1] = score_key(r.y, gi + 1);
      kk[4 * j + 2] = score_key(r.z, gi + 2);
      kk[4 * j + 3] = score_key(r.w, gi + 3);
    } else {
      kk[4 * j + 0] = kk[4 * j + 1] = kk[4 * j + 2] = kk[4 * j + 3] = 0ull;
    }
  }
}

// block-wide maximum through red[0..3]; every thread returns the same value
__device__ __forceinline__ unsigned long long lp_block_max(unsigned long long k,
                                                           unsigned long long* red) {
  k = wave_max_u64(k);
  __syncthreads();  // earlier reads of red are done
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = k;
  __syncthreads();
  k = red[0];
#pragma unroll
  for (int i = 1; i < kLpThreads / 64; ++i) k = umax64(k, red[i]);
  return k;
}

__global__ __launch_bounds__(kLpThreads) void logprob_topk_kernel(
    const float* __restrict__ logits, int V, int per, const int32_t* __restrict__ tokp,
    const int32_t* __restrict__ hist_len, int K, unsigned int* rec, int max_rec,
    unsigned long long* ws, unsigned int* ticket) {
  // [0..3] key reduce, [4..7] f64 sum reduce, [8] "this workgroup is the last"
  __shared__ unsigned long long sh[16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int G = gridDim.x, g = blockIdx.x;
  const float ninf = -__builtin_inff();
  const int c_lo = g * per, len = min(V - c_lo, per);  // c_lo < V: the grid is ceil(V / per)
  const bool one_piece = len <= kLpPiece;

  unsigned long long kk[kLpKeys];
  float M = ninf;
  double S = 0.0;
  unsigned long long best = 0ull;
  for (int o = 0; o < len; o += kLpPiece) {
    lp_load(logits + c_lo + o, min(len - o, kLpPiece), (unsigned int)(c_lo + o), tid, kk);
    unsigned long long k = kk[0];
#pragma unroll
    for (int i = 1; i < kLpKeys; ++i) k = umax64(k, kk[i]);
    k = lp_block_max(k, sh);
    best = umax64(best, k);
    const float mc = score_unordered((unsigned int)(k >> 32));
    if (mc == ninf) continue;  // a piece of -inf only adds nothing (uniform branch)
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < kLpKeys; ++i)
      if (kk[i] != 0ull) s += score_term(score_unordered((unsigned int)(kk[i] >> 32)), mc);
    s = wave_sum_f64(s);
    if (lane == 0) sh[4 + wave] = __builtin_bit_cast(unsigned long long, s);
    __syncthreads();
    double Sc = __builtin_bit_cast(double, sh[4]);
#pragma unroll
    for (int i = 1; i < kLpThreads / 64; ++i) Sc += __builtin_bit_cast(double, sh[4 + i]);
    // mc > -inf here, so the new maximum is finite
    const float Mn = fmaxf(M, mc);
    const double keep = M == ninf ? 0.0 : S * exp((double)M - (double)Mn);
    S = keep + Sc * exp((double)mc - (double)Mn);
    M = Mn;
  }

  // the slice's top K: round j finds the largest key below round j - 1's; thread j keeps it
  unsigned long long mine = tid == 0 ? best : 0ull;
  unsigned long long prev = best;
  for (int j = 1; j < K && prev != 0ull; ++j) {
    unsigned long long k = 0ull;
    for (int o = 0; o < len; o += kLpPiece) {
      if (!one_piece)
        lp_load(logits + c_lo + o, min(len - o, kLpPiece), (unsigned int)(c_lo + o), tid, kk);
#pragma unroll
      for (int i = 0; i < kLpKeys; ++i) k = umax64(k, kk[i] < prev ? kk[i] : 0ull);
    }
    k = lp_block_max(k, sh);
    if (tid == j) mine = k;
    prev = k;
  }

  unsigned long long* slot = ws + (size_t)g * kLpSlot;
  if (tid == 0) {
    slot[0] = __builtin_bit_cast(unsigned long long, S);
    slot[1] = (unsigned long long)__float_as_uint(M);
  }
  if (tid < K) slot[2 + tid] = mine;
  // publish the partial; the last workgroup folds all G of them (see the header)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned int drawn =
        __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const bool last = drawn == (unsigned int)(G - 1);
    if (last) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // re-arm
    }
    sh[8] = last ? 1ull : 0ull;
  }
  __syncthreads();
  if (sh[8] == 0ull) return;

  // row lse in wave 0: lane g holds slice g
  float lse = ninf;
  if (wave == 0) {
    float mg = ninf;
    double sg = 0.0;
    if (lane < G) {
      sg = __builtin_bit_cast(double, __builtin_nontemporal_load(ws + (size_t)lane * kLpSlot));
      mg = __uint_as_float(
          (unsigned int)__builtin_nontemporal_load(ws + (size_t)lane * kLpSlot + 1));
    }
    const float Mx = wave_max(mg);
    const double term = mg == ninf ? 0.0 : sg * exp((double)mg - (double)Mx);
    const double tot = wave_sum_f64(term);
    if (Mx != ninf && tot > 0.0) lse = (float)((double)Mx + log(tot));
  }

  // the top K of the G K candidates, five per thread at most
  constexpr int kCand = kLpMaxBlocks * kLpMaxK / kLpThreads;
  unsigned long long c[kCand];
  const int nc = G * K;
#pragma unroll
  for (int i = 0; i < kCand; ++i) {
    const int e = tid + i * kLpThreads;
    c[i] = e < nc ? __builtin_nontemporal_load(ws + (size_t)(e / K) * kLpSlot + 2 + (e % K))
                  : 0ull;
  }
  unsigned long long top = 0ull;
  prev = ~0ull;
  for (int j = 0; j < K && prev != 0ull; ++j) {
    unsigned long long k = 0ull;
#pragma unroll
    for (int i = 0; i < kCand; ++i) k = umax64(k, c[i] < prev ? c[i] : 0ull);
    k = lp_block_max(k, sh);
    if (tid == j) top = k;
    prev = k;
  }

  const int idx = *hist_len - 1;
  if (idx < 0 || idx >= max_rec) return;
  unsigned int* out = rec + (size_t)idx * kLpRecWords;
  if (tid < kLpMaxK) {  // threads 0..19: one top entry each
    const bool have = tid < K && top != 0ull;
    out[4 + tid] = have ? 0xffffffffu - (unsigned int)top : 0xffffffffu;
    out[24 + tid] = have ? __float_as_uint(score_unordered((unsigned int)(top >> 32)))
                         : __float_as_uint(ninf);
  } else if (tid >= 32 && tid < 36) {  // wave 0 holds lse in every lane
    const int tok = *tokp;
    unsigned int w;
    if (tid == 32) w = (unsigned int)tok;
    else if (tid == 33) w = tok >= 0 && tok < V ? __float_as_uint(logits[tok]) : 0x7fc00000u;
    else if (tid == 34) w = __float_as_uint(lse);
    else w = (unsigned int)K;
    out[tid - 32] = w;
  } else if (tid >= 36 && tid < 40) {
    out[44 + tid - 36] = 0u;
  }
}

// pieces of the row, and the slice length / grid for a cap on the workgroups
static inline void lp_plan(int V, int max_blocks, int* per, int* grid) {
  const int pieces = (V + kLpPiece - 1) / kLpPiece;
  const int cap = max_blocks > 0 && max_blocks < kLpMaxBlocks ? max_blocks : kLpMaxBlocks;
  const int g0 = pieces < cap ? pieces : cap;
  const long long p = (long long)((pieces + g0 - 1) / g0) * kLpPiece;
  *per = (int)(p > 0x7fffffffLL ? 0x7fffffffLL : p);
  *grid = (int)((V + p - 1) / p);
}

}  // namespace cake

using namespace cake;

// bytes of the partials workspace for a row of V logits (any max_blocks)
CAKE_API long long cake_logprob_ws_bytes(int V) {
  if (V < 1) return 0;
  int per, grid;
  lp_plan(V, 0, &per, &grid);
  return (long long)grid * kLpSlot * (long long)sizeof(unsigned long long);
}

// One record for the token *tok chosen from logits[V] (see the header).  ticket: one zeroed
// word, left zero by every launch; ws: cake_logprob_ws_bytes(V), 8-byte aligned; max_blocks
// 0: the default grid.
CAKE_API int cake_logprob_topk(const float* logits, int V, const int32_t* tok,
                               const int32_t* hist_len, int K, void* rec, int max_rec, void* ws,
                               unsigned int* ticket, int max_blocks, hipStream_t st) {
  if (!logits || !tok || !hist_len || !rec || !ws || !ticket || V < 1 || K < 0 || K > kLpMaxK ||
      max_rec < 1 || max_blocks < 0 || ((uintptr_t)logits & 3u) || ((uintptr_t)rec & 3u) ||
      ((uintptr_t)ws & 7u) || ((uintptr_t)ticket & 3u))
    return (int)hipErrorInvalidValue;
  int per, grid;
  lp_plan(V, max_blocks, &per, &grid);
  hipLaunchKernelGGL(logprob_topk_kernel, dim3(grid), dim3(kLpThreads), 0, st, logits, V, per, tok,
                     hist_len, K, static_cast<unsigned int*>(rec), max_rec,
                     static_cast<unsigned long long*>(ws), ticket);
  return (int)hipGetLastError();
}
