// Sequence scoring: a streaming log-sum-exp, target gather and argmax over the rows of an
// f32 logit block that holds one chunk [v0, v0 + Vc) of the vocabulary.
//
// State per row, carried from chunk to chunk (any order):
//   run_max  m   f32   the largest logit seen (-inf before the first chunk)
//   run_sum  S   f64   sum exp(x - m) over the logits seen
//   tgt          f32   the logit of target[t], copied bit for bit by the chunk that holds it
//   key          u64   (ordered_key(x) << 32) | ~(v0 + j): the head-select key of
//                      gemv_kernel.h, so the maximum is the largest logit with the lowest
//                      vocabulary id at ties, across chunks too
// Merge: m' = max(m, mc); S' = S exp(m - m') + Sc exp(mc - m'), an -inf maximum counting 0
// (so (-inf) - (-inf) is never evaluated).  Finish: lse = m + log(S).
//
// Arithmetic: exp is v_exp_f32 of (x - m) * log2(e) in f32; every addition into the sum is
// f64, per lane and across lanes (as the f64 partials of gn_nhwc_stats_kernel); the merge
// and the final log are f64.  A term's relative error is then at most (2 |d| + 2) 2^-24
// with d = x - m, which bounds |lse - exact| by 2^-24 (|exact| + 64) for V <= 2^17.
//
// One workgroup of 256 threads per row.  A piece of up to 8192 columns stays in registers
// between the maximum and the sum (the logits are read once, as quant_fp8.hip holds its row
// between amax and convert); longer chunks loop over pieces with the same merge.  The row's
// 16-byte aligned middle is read with 16-byte loads, up to three leading and three trailing
// columns with scalar loads, whatever the base and ld are.
#include "common.h"
#include "reduce64.h"

namespace cake {

constexpr int kScoreThreads = 256;
constexpr int kScoreNV = 8;                                  // 16-byte loads per thread
constexpr int kScorePiece = kScoreThreads * kScoreNV * 4;    // 8192 columns

__global__ __launch_bounds__(kScoreThreads) void lse_rows_kernel(
    const float* __restrict__ logits, long long ld, int Vc, int v0, int first,
    const int32_t* __restrict__ target, float* __restrict__ run_max, double* __restrict__ run_sum,
    float* __restrict__ tgt, unsigned long long* __restrict__ key) {
  __shared__ unsigned long long red_k[kScoreThreads / 64];
  __shared__ double red_s[kScoreThreads / 64];
  const int t = blockIdx.x, tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const float* row = logits + (size_t)t * (size_t)ld;
  const float ninf = -__builtin_inff();

  float M = ninf;
  double S = 0.0;
  unsigned long long best = 0ull;
  if (!first) {
    M = run_max[t];
    S = run_sum[t];
    best = key[t];
  }
  if (tid == 0) {
    const int tg = target[t];
    if (first) tgt[t] = __uint_as_float(0x7fc00000u);
    if (tg >= v0 && tg - v0 < Vc) tgt[t] = row[tg - v0];
  }

  for (int p0 = 0; p0 < Vc; p0 += kScorePiece) {
    const float* src = row + p0;
    const int n = min(Vc - p0, kScorePiece);
    // columns [0, lead) and [lead + 4 nvec, n) are read one by one, the rest 16 bytes each
    const int lead = min(n, (int)(((16u - (unsigned int)((uintptr_t)src & 15u)) & 15u) >> 2));
    const int nvec = (n - lead) >> 2;
    const int ntail = n - lead - 4 * nvec;
    const unsigned int g0 = (unsigned int)(v0 + p0);

    float4 r[kScoreNV];
    float xs = ninf;
    int cs = -1;  // this thread's scalar column, if it has one (lead + ntail <= 6)
    if (tid < lead) cs = tid;
    else if (tid < lead + ntail) cs = lead + 4 * nvec + (tid - lead);
    unsigned long long k = 0ull;
    if (cs >= 0) {
      xs = src[cs];
      k = score_key(xs, g0 + (unsigned int)cs);
    }
#pragma unroll
    for (int j = 0; j < kScoreNV; ++j) {
      const int c = j * kScoreThreads + tid;
      r[j] = make_float4(ninf, ninf, ninf, ninf);
      if (c < nvec) {
        r[j] = *reinterpret_cast<const float4*>(src + lead + 4 * c);
        const unsigned int gi = g0 + (unsigned int)(lead + 4 * c);
        k = umax64(k, score_key(r[j].x, gi));
        k = umax64(k, score_key(r[j].y, gi + 1));
        k = umax64(k, score_key(r[j].z, gi + 2));
        k = umax64(k, score_key(r[j].w, gi + 3));
      }
    }
    k = wave_max_u64(k);
    __syncthreads();  // the previous piece's reads of red_k / red_s are done
    if (lane == 0) red_k[wave] = k;
    __syncthreads();
    k = red_k[0];
#pragma unroll
    for (int i = 1; i < kScoreThreads / 64; ++i) k = umax64(k, red_k[i]);
    best = umax64(best, k);
    const float mc = score_unordered((unsigned int)(k >> 32));
    if (mc == ninf) continue;  // a piece of -inf only adds nothing (uniform branch)

    double s = 0.0;
    if (cs >= 0) s += score_term(xs, mc);
#pragma unroll
    for (int j = 0; j < kScoreNV; ++j) {
      // slots past the piece hold -inf: their terms are exactly 0
      s += score_term(r[j].x, mc);
      s += score_term(r[j].y, mc);
      s += score_term(r[j].z, mc);
      s += score_term(r[j].w, mc);
    }
    s = wave_sum_f64(s);
    if (lane == 0) red_s[wave] = s;
    __syncthreads();
    double Sc = red_s[0];
#pragma unroll
    for (int i = 1; i < kScoreThreads / 64; ++i) Sc += red_s[i];
    // mc > -inf here, so the new maximum is finite
    const float Mn = fmaxf(M, mc);
    const double keep = M == ninf ? 0.0 : S * exp((double)M - (double)Mn);
    S = keep + Sc * exp((double)mc - (double)Mn);
    M = Mn;
  }

  if (tid == 0) {
    run_max[t] = M;
    run_sum[t] = S;
    key[t] = best;
  }
}

__global__ __launch_bounds__(256) void lse_finish_kernel(
    const float* __restrict__ run_max, const double* __restrict__ run_sum,
    const unsigned long long* __restrict__ key, int T, float* __restrict__ lse,
    int32_t* __restrict__ top, float* __restrict__ topv) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= T) return;
  const float m = run_max[t];
  const double S = run_sum[t];
  const float ninf = -__builtin_inff();
  lse[t] = (m == ninf || !(S > 0.0)) ? ninf : (float)((double)m + log(S));
  const unsigned long long k = key[t];
  top[t] = k == 0ull ? 0 : (int32_t)(0xffffffffu - (unsigned int)k);
  topv[t] = k == 0ull ? ninf : score_unordered((unsigned int)(k >> 32));
}

}  // namespace cake

using namespace cake;

// logits[t * ld + j]: the logit of vocabulary id v0 + j (j < Vc) of row t.  first != 0
// starts the rows' state; target[t] = -1: no target (tgt[t] stays NaN).
CAKE_API int cake_lse_rows(const float* logits, long long ld, int T, int Vc, int v0, int first,
                           const int32_t* target, float* run_max, double* run_sum, float* tgt,
                           unsigned long long* key, hipStream_t st) {
  if (!logits || !target || !run_max || !run_sum || !tgt || !key || T < 1 || Vc < 1 || v0 < 0 ||
      ld < Vc || (long long)v0 + Vc > 0x7fffffffLL || ((uintptr_t)logits & 3u))
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(lse_rows_kernel, dim3(T), dim3(kScoreThreads), 0, st, logits, ld, Vc, v0,
                     first, target, run_max, run_sum, tgt, key);
  return (int)hipGetLastError();
}

CAKE_API int cake_lse_finish(const float* run_max, const double* run_sum,
                             const unsigned long long* key, int T, float* lse, int32_t* top,
                             float* topv, hipStream_t st) {
  if (!run_max || !run_sum || !key || !lse || !top || !topv || T < 1)
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(lse_finish_kernel, dim3((T + 255) / 256), dim3(256), 0, st, run_max, run_sum,
                     key, T, lse, top, topv);
  return (int)hipGetLastError();
}
