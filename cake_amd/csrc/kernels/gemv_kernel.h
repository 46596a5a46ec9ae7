// Decode GEMV kernels and their launchers: one kernel family over a weight-format policy F
// (W16 below, W8 in gemv_w8_kernel.h, W4 in gemv_w4_kernel.h, P13 in gemv_p13_kernel.h).
// The C entry points are spread over gemv*.hip so the many (format, dtype, U, prefetch, NX)
// instantiations compile in parallel.  Design notes: gemv.hip.  One (kind, format) is not of
// the family: the MXFP4 16-bit-input GEMV keeps its own kernel and pair loop
// (gemv_w4_x16.hip says why).
#pragma once
#include <type_traits>

#include "common.h"

namespace cake {

constexpr int kGemvThreads = 256;  // 4 waves
constexpr int kGemvWaves = kGemvThreads / 64;
constexpr int kGemvMaxBlocks = 1024;

typedef float f32x2_t __attribute__((ext_vector_type(2)));  // as mxfp4.h

// Launch geometry per kernel kind (tunable at run time; defaults from the
// rocprofv3-measured sweeps in profiles/): U = chunks in flight per row,
// PF = prefetch the first weight batch before the x prologue, MB = grid cap.
struct GemvTune { int U, PF, MB; };
// kX16 = 16-bit-input GEMVs (W16: those with K > 8192, down_proj), kX16S = W16 with
// K <= 8192 (o_proj); the quantised formats have the first four kinds
enum GemvKind { kQkv = 0, kSwiglu = 1, kX16 = 2, kNormF32 = 3, kX16S = 4, kNumKinds = 5 };
// the run-time tuning tables [F::kFmt][kind] (defined in gemv.hip, set by cake_gemv*_set_tuning)
extern GemvTune g_tune[4][kNumKinds];

// ---------------------------------------------------------------------------
// Weight formats.  A policy F supplies what differs between the formats:
//   kFmt, kKinds          its row of g_tune and how many kinds of it exist
//   kLog2                 log2 of the k values in a lane's 16-byte chunk
//   kPad32, kPad16        the LDS x row (f32 / 16-bit) holds K rounded up to this many values
//   perm32(i), perm16(i)  where value i of the f32 / 16-bit x row sits in LDS
//   kU[3], kPF[2]         the U values and the non-zero prefetch depths (deepest first) that are
//                         instantiated: what *_set_tuning accepts (besides prefetch 0)
//   prefetch(pf, K)       the prefetch depth a row of K values runs with
//   kStrict               launchers refuse K < one chunk and empty outputs
//   Acc, zero(), total()  a row's per-lane accumulator, and its sum before wave_sum
//   Mat, pick()           the matrix handle (a kernel argument) and the QKV matrix of a pair
//   kRowScale             Mat has one f32 `scale` per row, applied to the wave sums
//   Rows, rows()          the pair of rows a wave works on
//   Chunk, load<NT>()     one chunk of both rows (NT: non-temporal, the main loop)
//   fma<DT, XF32>()       acc += chunk . x
//   kRawRows (optional)   Rows carries per-row state read from memory (run_pairs takes a wave's
//                         first rows from the prefetch registers, not from a second map()), and
//                         is_raw() / raw_rows(): a pair kept as plain 16-bit rows runs W16's loop
// ---------------------------------------------------------------------------

// the q / k / v pointer of pair kind 0 / 1 / 2 by address arithmetic, not a pointer select:
// a select between kernel-argument fields becomes a memory load of the argument block, which
// would stand (in vmcnt order) in front of the split prologue's x loads (offsets from q keep
// the global address space visible: no flat loads)
template <class T>
__device__ __forceinline__ const T* pick3(const T* q, const T* k, const T* v, int kind) {
  const ptrdiff_t dk = k - q, dv = v - q;  // both read ahead of the select
  return q + (kind == 0 ? 0 : (kind == 1 ? dk : dv));
}

// rows of 16-byte chunks with nothing beside them (W16, W8)
struct PlainRows {
  struct Rows { const uint4 *a, *b; };
  struct Chunk { uint4 a, b; };
  template <bool NT> static __device__ __forceinline__ Chunk load(const Rows& r, int c) {
    if constexpr (NT) return {ld_nt16(r.a + c), ld_nt16(r.b + c)};
    else return {r.a[c], r.b[c]};
  }
  // PF falls back to 0 when a row is shorter than PF*64 chunks (small test shapes)
  template <int LOG2> static int prefetch_if_filled(int pf, int K) {
    return (K >> LOG2) >= 64 * pf ? pf : 0;
  }
};

template <int DT, bool XF32>
__device__ __forceinline__ void load_x8(const void* xs, int chunk, float* o) {
  if constexpr (XF32) {
    const float4* p = reinterpret_cast<const float4*>(xs) + chunk * 2;
    const float4 a = p[0], b = p[1];
    o[0] = a.x; o[1] = a.y; o[2] = a.z; o[3] = a.w;
    o[4] = b.x; o[5] = b.y; o[6] = b.z; o[7] = b.w;
  } else {
    unpack8<DT>(reinterpret_cast<const uint4*>(xs)[chunk], o);
  }
}

// 16-bit weights [N, K]: 8 k values per chunk, a scalar fmaf chain per row
struct W16 : PlainRows {
  static constexpr int kFmt = 0, kKinds = kNumKinds, kLog2 = 3, kPad32 = 1, kPad16 = 1;
  static constexpr int kU[3] = {2, 4, 8}, kPF[2] = {8, 4};
  static constexpr bool kStrict = false, kRowScale = false;
  static __device__ __forceinline__ int perm32(int i) { return i; }
  static __device__ __forceinline__ int perm16(int i) { return i; }
  static int prefetch(int pf, int K) { return prefetch_if_filled<kLog2>(pf, K); }
  using Acc = float;
  static __device__ __forceinline__ Acc zero() { return 0.f; }
  static __device__ __forceinline__ float total(Acc a) { return a; }
  struct Mat { const uint16_t* w; };
  static __device__ __forceinline__ Mat pick(const Mat& q, const Mat& k, const Mat& v, int kind) {
    return {pick3(q.w, k.w, v.w, kind)};
  }
  static __device__ __forceinline__ Rows rows(const Mat& ma, size_t ra, const Mat& mb, size_t rb,
                                              int K) {
    return {reinterpret_cast<const uint4*>(ma.w + ra * K),
            reinterpret_cast<const uint4*>(mb.w + rb * K)};
  }
  template <int DT, bool XF32>
  static __device__ __forceinline__ void fma(const void* xs, int chunk, const Chunk& v, Acc& acc_a,
                                             Acc& acc_b) {
    float xv[8], fa[8], fb[8];
    load_x8<DT, XF32>(xs, chunk, xv);
    unpack8<DT>(v.a, fa);
    unpack8<DT>(v.b, fb);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      acc_a = fmaf(fa[e], xv[e], acc_a);
      acc_b = fmaf(fb[e], xv[e], acc_b);
    }
  }
};

template <class F, class = void> struct HasRawRows : std::false_type {};
template <class F>
struct HasRawRows<F, std::void_t<decltype(F::kRawRows)>> : std::bool_constant<F::kRawRows> {};

template <class F, class = void> struct Bf16Only : std::false_type {};
template <class F>
struct Bf16Only<F, std::void_t<decltype(F::kBf16Only)>> : std::bool_constant<F::kBf16Only> {};

// The occupancy (waves per SIMD) the register allocator is asked to keep for the 16-bit-input
// GEMV of a format at U chunks in flight: x16_waves(U) where the format has one, else 1, the
// compiler's own floor.
template <class F, int U, class = void> struct X16Waves : std::integral_constant<int, 1> {};
template <class F, int U>
struct X16Waves<F, U, std::void_t<decltype(F::x16_waves(U))>>
    : std::integral_constant<int, F::x16_waves(U)> {};

// The epilogue scale hook.  kRowScale (fp8): the first pair's row scales are requested in
// the prologue slot (row_scale) and every wave sum is multiplied by its row's (descale);
// nothing for the other formats.
template <class F>
__device__ __forceinline__ float row_scale(const typename F::Mat& m, size_t row) {
  if constexpr (F::kRowScale) return m.scale[row];
  else return 1.f;
}
template <class F>
__device__ __forceinline__ float descale(float d, bool first, float s0, const typename F::Mat& m,
                                         size_t row) {
  if constexpr (F::kRowScale) return d * (first ? s0 : m.scale[row]);
  else return d;
}

// ---------------------------------------------------------------------------
// x staging (prologues)
// ---------------------------------------------------------------------------

// Normalise a f32 row into LDS:  xs[i] = x[i] * rsqrt(mean(x^2) + eps) * w[i].
template <class F, int DT>
__device__ __forceinline__ void stage_rmsnorm(const float* __restrict__ x,
                                              const uint16_t* __restrict__ w,
                                              float eps, int K, float* xs) {
  __shared__ float red[16];
  float ss = 0.f;
  for (int i = threadIdx.x * 4; i < K; i += kGemvThreads * 4) {
    const float4 v = *reinterpret_cast<const float4*>(x + i);
    *reinterpret_cast<float4*>(xs + F::perm32(i)) = v;
    ss += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
  }
  ss = block_sum(ss, red);
  const float r = rsqrtf(ss / (float)K + eps);
  for (int i = threadIdx.x * 4; i < K; i += kGemvThreads * 4) {
    float4 v = *reinterpret_cast<float4*>(xs + F::perm32(i));
    const uint2 wv = *reinterpret_cast<const uint2*>(w + i);
    v.x *= r * to_f32<DT>((uint16_t)(wv.x & 0xffff));
    v.y *= r * to_f32<DT>((uint16_t)(wv.x >> 16));
    v.z *= r * to_f32<DT>((uint16_t)(wv.y & 0xffff));
    v.w *= r * to_f32<DT>((uint16_t)(wv.y >> 16));
    *reinterpret_cast<float4*>(xs + F::perm32(i)) = v;
  }
  __syncthreads();
}

// Copy a 16-bit activation row into LDS (kept 16-bit: 70B down_proj has K=28672).
template <class F>
__device__ __forceinline__ void stage_plain16(const uint16_t* __restrict__ x, int K,
                                              uint16_t* xs) {
  for (int i = threadIdx.x * 8; i < K; i += kGemvThreads * 8)
    *reinterpret_cast<uint4*>(xs + F::perm16(i)) = *reinterpret_cast<const uint4*>(x + i);
  __syncthreads();
}

// Split x prologues (NX > 0, used with a weight prefetch PFC > 0): the x loads
// are issued FIRST, then the wave's first weight rows, then the x half is
// finished.  Loads retire in order (vmcnt), so issuing the weights first — the
// plain prologue order — made the norm wait for the whole weight batch; in this
// order the norm waits only for x, and its reduction / LDS round trips overlap
// the weight stream.  K = 1024 NX (RMSNorm, f32 row) or 2048 NX (16-bit row).
template <class F, int DT, int NX> struct NormPre {  // K <= 1024 NX, K % 4 == 0
  float4 x[NX];
  uint2 w[NX];
  __device__ __forceinline__ void load(const float* __restrict__ xg, const uint16_t* __restrict__ wg,
                                       int K) {
#pragma unroll
    for (int j = 0; j < NX; ++j) {
      const int i = (j * kGemvThreads + threadIdx.x) * 4;
      x[j] = i < K ? *reinterpret_cast<const float4*>(xg + i) : make_float4(0.f, 0.f, 0.f, 0.f);
      w[j] = i < K ? *reinterpret_cast<const uint2*>(wg + i) : make_uint2(0u, 0u);
    }
  }
  __device__ __forceinline__ void finish(float eps, int K, float* xs) {
    __shared__ float red[16];
    float ss = 0.f;
#pragma unroll
    for (int j = 0; j < NX; ++j) ss += x[j].x * x[j].x + x[j].y * x[j].y + x[j].z * x[j].z + x[j].w * x[j].w;
    ss = block_sum(ss, red);
    const float r = rsqrtf(ss / (float)K + eps);
#pragma unroll
    for (int j = 0; j < NX; ++j) {
      const int i = (j * kGemvThreads + threadIdx.x) * 4;
      float4 v = x[j];
      v.x *= r * to_f32<DT>((uint16_t)(w[j].x & 0xffff));
      v.y *= r * to_f32<DT>((uint16_t)(w[j].x >> 16));
      v.z *= r * to_f32<DT>((uint16_t)(w[j].y & 0xffff));
      v.w *= r * to_f32<DT>((uint16_t)(w[j].y >> 16));
      if (i < K) *reinterpret_cast<float4*>(xs + F::perm32(i)) = v;
    }
    __syncthreads();
  }
};

template <class F, int NX> struct Plain16Pre {  // K <= 2048 NX, K % 8 == 0
  uint4 v[NX];
  __device__ __forceinline__ void load(const uint16_t* __restrict__ xg, int K) {
#pragma unroll
    for (int j = 0; j < NX; ++j) {
      const int i = (j * kGemvThreads + threadIdx.x) * 8;
      v[j] = i < K ? *reinterpret_cast<const uint4*>(xg + i) : make_uint4(0u, 0u, 0u, 0u);
    }
  }
  __device__ __forceinline__ void finish(int K, uint16_t* xs) {
#pragma unroll
    for (int j = 0; j < NX; ++j) {
      const int i = (j * kGemvThreads + threadIdx.x) * 8;
      if (i < K) *reinterpret_cast<uint4*>(xs + F::perm16(i)) = v[j];
    }
    __syncthreads();
  }
};

// ---------------------------------------------------------------------------
// core: one wave computes dot products of a PAIR of weight rows with the x row
// staged in LDS.  U = 16-byte chunks per row in flight per lane per iteration
// (2*U loads outstanding).  PFC = chunks per row per lane of the wave's FIRST
// pair issued before the x prologue (RMSNorm / staging) so the HBM stream
// overlaps it; for 16-bit K = 4096 PFC = 8 is the whole pair (64 VGPRs).  All
// register arrays are indexed by compile-time constants (no scratch).
// ---------------------------------------------------------------------------

// accumulate chunks [c_start, nch) of the pair (c_start a multiple of 64)
template <class F, int DT, bool XF32, int U>
__device__ __forceinline__ void dot_range(const typename F::Rows& r, const void* xs, int nch,
                                          int c_start, typename F::Acc& acc_a,
                                          typename F::Acc& acc_b) {
  const int lane = threadIdx.x & 63;
  const int full = c_start + ((nch - c_start) / (64 * U)) * (64 * U);
  for (int c0 = c_start; c0 < full; c0 += 64 * U) {
    typename F::Chunk v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) v[u] = F::template load<true>(r, c0 + u * 64 + lane);
#pragma unroll
    for (int u = 0; u < U; ++u) F::template fma<DT, XF32>(xs, c0 + u * 64 + lane, v[u], acc_a, acc_b);
  }
  // the tail: lanes past nch have no chunk
  for (int c = full + lane; c < nch; c += 64)
    F::template fma<DT, XF32>(xs, c, F::template load<false>(r, c), acc_a, acc_b);
}

// prefetch registers: PFC chunks of the pair per lane
template <class F, int PFC, bool RAW = HasRawRows<F>::value> struct Regs {
  typename F::Chunk c[PFC > 0 ? PFC : 1];
};
template <class F, int PFC> struct Regs<F, PFC, true> {
  typename F::Chunk c[PFC > 0 ? PFC : 1];
  typename F::Rows r;  // the rows prefetch_rows was given
};

// issue the first PFC chunks of the pair (nch >= 64 PFC)
template <class F, int PFC>
__device__ __forceinline__ void prefetch_rows(const typename F::Rows& r, Regs<F, PFC>& g) {
  if constexpr (PFC > 0) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int c = 0; c < PFC; ++c) g.c[c] = F::template load<true>(r, c * 64 + lane);
  }
}

// kRawRows: keep the (clamped) first pair's rows, whose headers are already requested, for
// run_pairs_raw.  Every wave does, prefetching or not: choosing between these rows and fresh
// ones there made the compiler pick through memory (48 bytes of scratch per lane).
template <class F, int PFC>
__device__ __forceinline__ void keep_rows(const typename F::Rows& r, Regs<F, PFC>& g) {
  if constexpr (HasRawRows<F>::value) g.r = r;
}

// run_pairs of a kRawRows format.  A pair kept as plain 16-bit rows takes its dot products
// from W16's loop (the same per-lane order whatever W16's U); the branch is wave-uniform and
// stands once per pair, in front of two complete code paths, each with its own epilogue call.
// A pair's rows (its headers) are asked for one pair ahead, while the pair before streams.
template <class F, int DT, bool XF32, int U, int PFC, class Map, class Epi>
__device__ __forceinline__ void run_pairs_raw(const Map& map, const Epi& epi, const void* xs, int K,
                                              int npairs, int p0, int stride,
                                              const Regs<F, PFC>& pre) {
  const int nch = K >> F::kLog2;
  auto raw_dots = [&](const typename F::Rows& r, float& aa, float& ab) {
    dot_range<W16, DT, XF32, 4>(F::raw_rows(r, K), xs, K >> W16::kLog2, 0, aa, ab);
  };
  auto clamped = [&](int q) { return map(q < npairs ? q : npairs - 1); };
  int p = p0;
  typename F::Rows rn;
  if constexpr (PFC > 0) {
    // the rows keep_rows was given: the wave's first pair, clamped (an idle wave of a kernel
    // without the split prologue has prefetched nothing: it works on the last pair and drops it)
    const typename F::Rows r = pre.r;
    rn = clamped(p + stride);
    const int lane = threadIdx.x & 63;
    if (F::is_raw(r)) {  // (the prefetched planes are dropped)
      float aa = 0.f, ab = 0.f;
      raw_dots(r, aa, ab);
      const float sa = wave_sum(aa), sb = wave_sum(ab);
      if (p < npairs) epi(p, sa, sb);
    } else {
      typename F::Acc aa = F::zero(), ab = F::zero();
#pragma unroll
      for (int c = 0; c < PFC; ++c) F::template fma<DT, XF32>(xs, c * 64 + lane, pre.c[c], aa, ab);
      dot_range<F, DT, XF32, U>(r, xs, nch, PFC * 64, aa, ab);
      const float sa = wave_sum(F::total(aa)), sb = wave_sum(F::total(ab));
      if (p < npairs) epi(p, sa, sb);
    }
    p += stride;
  } else {
    rn = clamped(p);
  }
  for (; p < npairs; p += stride) {
    const typename F::Rows r = rn;
    rn = clamped(p + stride);
    if (F::is_raw(r)) {
      float aa = 0.f, ab = 0.f;
      raw_dots(r, aa, ab);
      epi(p, wave_sum(aa), wave_sum(ab));
      continue;
    }
    typename F::Acc aa = F::zero(), ab = F::zero();
    dot_range<F, DT, XF32, U>(r, xs, nch, 0, aa, ab);
    epi(p, wave_sum(F::total(aa)), wave_sum(F::total(ab)));
  }
}

// Walk the wave's pairs p0, p0+stride, ...: map(p) gives the rows, epi(p, da, db)
// consumes the two dot products (full wave sums; kRowScale: not yet scaled).
template <class F, int DT, bool XF32, int U, int PFC, class Map, class Epi>
__device__ __forceinline__ void run_pairs(const Map& map, const Epi& epi, const void* xs, int K,
                                          int npairs, int p0, int stride,
                                          const Regs<F, PFC>& pre) {
  if constexpr (HasRawRows<F>::value) {
    run_pairs_raw<F, DT, XF32, U, PFC>(map, epi, xs, K, npairs, p0, stride, pre);
    return;
  }
  const int nch = K >> F::kLog2;
  int p = p0;
  if constexpr (PFC > 0) {
    // Unconditional (an idle wave works on a clamped pair and drops it): a use of
    // the prefetched registers inside a branch lets the compiler sink the
    // prefetch loads past the x prologue's barrier, serialising them again.
    const typename F::Rows r = map(p < npairs ? p : npairs - 1);
    const int lane = threadIdx.x & 63;
    typename F::Acc aa = F::zero(), ab = F::zero();
#pragma unroll
    for (int c = 0; c < PFC; ++c) F::template fma<DT, XF32>(xs, c * 64 + lane, pre.c[c], aa, ab);
    dot_range<F, DT, XF32, U>(r, xs, nch, PFC * 64, aa, ab);
    const float sa = wave_sum(F::total(aa)), sb = wave_sum(F::total(ab));
    if (p < npairs) epi(p, sa, sb);
    p += stride;
  }
  for (; p < npairs; p += stride) {
    const typename F::Rows r = map(p);
    typename F::Acc aa = F::zero(), ab = F::zero();
    dot_range<F, DT, XF32, U>(r, xs, nch, 0, aa, ab);
    epi(p, wave_sum(F::total(aa)), wave_sum(F::total(ab)));
  }
}

// ---------------------------------------------------------------------------
// QKV + RoPE + KV-cache write
// ---------------------------------------------------------------------------
template <class F> struct QkvArgs {
  const float* resid;      // [K] f32
  const uint16_t* norm_w;  // [K]
  float eps;
  typename F::Mat q, k, v;  // [nh*hd, K], [nkv*hd, K], [nkv*hd, K]
  int K, nh, nkv, hd;
  const float* inv_freq;  // [hd/2]
  const int* pos;         // device scalar: position of this token
  float* q_out;           // [nh*hd] f32 (roped)
  uint16_t* kcache;       // [nkv][S][hd] (this layer)
  uint16_t* vcache;
  int S;
  int kv_fmt;             // KvFmt of the cache (common.h); 1: kcache / vcache hold bytes
};

// pair p of the fused projection: rows (ra, ra + hd/2) of head `head` of its matrix
struct QkvPair {
  int kind, head, i;  // kind 0 = q, 1 = k, 2 = v; i = the pair's RoPE frequency
  size_t ra;
};

__device__ __forceinline__ QkvPair qkv_pair(int p, int half, int nh, int nqk, int hd) {
  const int slot = p / half;
  const bool isq = slot < nh, isk = !isq && slot < nqk;
  QkvPair r;
  r.kind = isq ? 0 : (isk ? 1 : 2);
  r.head = slot - (isq ? 0 : (isk ? nh : nqk));
  r.i = p - slot * half;
  r.ra = (size_t)r.head * hd + r.i;
  return r;
}

template <class F, int DT, int U, int PFC, int NX>
__global__ __launch_bounds__(kGemvThreads) void qkv_rope_kernel(QkvArgs<F> a) {
  extern __shared__ float xs[];
  const int half = a.hd >> 1;
  const int npairs = (a.nh + 2 * a.nkv) * half;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int p0 = blockIdx.x * kGemvWaves + wave;
  const int nh = a.nh, nqk = a.nh + a.nkv, hd = a.hd, K = a.K;
  auto map = [&](int p) {
    const QkvPair r = qkv_pair(p, half, nh, nqk, hd);
    const typename F::Mat m = F::pick(a.q, a.k, a.v, r.kind);  // by address arithmetic: pick3
    return F::rows(m, r.ra, m, r.ra + half, K);
  };
  Regs<F, PFC> pre;
  NormPre<F, DT, NX> xp;
  const int pc = p0 < npairs ? p0 : npairs - 1;
  const typename F::Rows r0 = map(pc);  // rows first: their address math may load (kernarg select)
  keep_rows<F, PFC>(r0, pre);
  if constexpr (NX > 0) xp.load(a.resid, a.norm_w, a.K);
  __builtin_amdgcn_sched_barrier(0);  // x loads strictly before the weights (in-order vmcnt)
  if (NX > 0 || (PFC > 0 && p0 < npairs)) prefetch_rows<F, PFC>(r0, pre);  // NX: exact vmcnt
  // the epilogue operands of the wave's first pair, requested now: the RoPE frequency
  // (loaded in the epilogue it was one more memory round trip at the end of every wave)
  // and the row scales
  const QkvPair rc = qkv_pair(pc, half, nh, nqk, hd);
  const float f0 = a.inv_freq[rc.i];
  const typename F::Mat mc = F::pick(a.q, a.k, a.v, rc.kind);
  const float s0a = row_scale<F>(mc, rc.ra), s0b = row_scale<F>(mc, rc.ra + half);
  __builtin_amdgcn_sched_barrier(0);
  if constexpr (NX > 0) xp.finish(a.eps, a.K, xs);
  else stage_rmsnorm<F, DT>(a.resid, a.norm_w, a.eps, a.K, xs);
  const int pos = *a.pos;
  auto epi = [&](int p, float da, float db) {
    if (lane != 0) return;
    const QkvPair r = qkv_pair(p, half, nh, nqk, hd);
    const typename F::Mat m = F::pick(a.q, a.k, a.v, r.kind);
    if constexpr (F::kRowScale) {
      float sa = s0a, sb = s0b;
      if (p != p0) { sa = m.scale[r.ra]; sb = m.scale[r.ra + half]; }
      da *= sa;
      db *= sb;
    }
    float oa = da, ob = db;
    if (r.kind < 2) {
      float s, c;
      sincosf((float)pos * (p == p0 ? f0 : a.inv_freq[r.i]), &s, &c);
      oa = da * c - db * s;
      ob = da * s + db * c;
    }
    if (r.kind == 0) {
      a.q_out[r.ra] = oa;
      a.q_out[r.ra + half] = ob;
    } else {
      uint16_t* cache = r.kind == 1 ? a.kcache : a.vcache;
      const size_t off = ((size_t)r.head * a.S + pos) * a.hd + r.i;
      kv_store_pair<DT>(cache, off, half, oa, ob, a.kv_fmt);
    }
  };
  run_pairs<F, DT, true, U, PFC>(map, epi, xs, a.K, npairs, p0, gridDim.x * kGemvWaves, pre);
}

// ---------------------------------------------------------------------------
// RMSNorm + gate/up + SiLU*mul
// ---------------------------------------------------------------------------
template <class F, int DT, int U, int PFC, int NX>
__global__ __launch_bounds__(kGemvThreads) void swiglu_kernel(
    const float* __restrict__ resid, const uint16_t* __restrict__ norm_w, float eps,
    const typename F::Mat wg, const typename F::Mat wu, int K, int I,
    uint16_t* __restrict__ act) {
  extern __shared__ float xs[];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int j0 = blockIdx.x * kGemvWaves + wave;
  auto map = [&](int j) { return F::rows(wg, (size_t)j, wu, (size_t)j, K); };
  Regs<F, PFC> pre;
  NormPre<F, DT, NX> xp;
  const int jp = j0 < I ? j0 : I - 1;
  const typename F::Rows r0 = map(jp);
  keep_rows<F, PFC>(r0, pre);
  if constexpr (NX > 0) xp.load(resid, norm_w, K);
  __builtin_amdgcn_sched_barrier(0);  // x loads strictly before the weights (in-order vmcnt)
  // NX: unconditional (an idle wave re-reads the last row), so the vmcnt is exact
  if (NX > 0 || (PFC > 0 && j0 < I)) prefetch_rows<F, PFC>(r0, pre);
  const float s0g = row_scale<F>(wg, jp), s0u = row_scale<F>(wu, jp);  // requested now
  __builtin_amdgcn_sched_barrier(0);
  if constexpr (NX > 0) xp.finish(eps, K, xs);
  else stage_rmsnorm<F, DT>(resid, norm_w, eps, K, xs);
  auto epi = [&](int j, float g, float u) {
    if (lane != 0) return;
    g = descale<F>(g, j == j0, s0g, wg, j);
    u = descale<F>(u, j == j0, s0u, wu, j);
    act[j] = from_f32<DT>(silu(g) * u);
  };
  run_pairs<F, DT, true, U, PFC>(map, epi, xs, K, I, j0, gridDim.x * kGemvWaves, pre);
}

// ---------------------------------------------------------------------------
// out (+)= W x   with 16-bit x: o_proj / down_proj (accumulate into the f32
// residual stream) — or plain f32 output.
// ---------------------------------------------------------------------------
template <class F, int DT, int U, int PFC, int NX, bool ACCUM>
__global__ __launch_bounds__(kGemvThreads) __attribute__((amdgpu_waves_per_eu(X16Waves<F, U>::value)))
void gemv_x16_kernel(
    const uint16_t* __restrict__ x, const typename F::Mat w, int K, int N,
    float* __restrict__ out) {
  extern __shared__ float smem[];
  uint16_t* xs = reinterpret_cast<uint16_t*>(smem);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int npairs = (N + 1) >> 1;
  const int p0 = blockIdx.x * kGemvWaves + wave;
  auto map = [&](int p) { return F::rows(w, (size_t)(2 * p), w, (size_t)min(2 * p + 1, N - 1), K); };
  Regs<F, PFC> pre;
  Plain16Pre<F, NX> xp;
  const int pc = p0 < npairs ? p0 : npairs - 1;
  const typename F::Rows r0 = map(pc);
  keep_rows<F, PFC>(r0, pre);
  if constexpr (NX > 0) xp.load(x, K);
  __builtin_amdgcn_sched_barrier(0);  // x loads strictly before the weights (in-order vmcnt)
  if (NX > 0 || (PFC > 0 && p0 < npairs)) prefetch_rows<F, PFC>(r0, pre);  // NX: exact vmcnt
  // the epilogue operands of the wave's first pair, requested now: the row scales and
  // (ACCUM) the residual words (read in the epilogue they were one more memory round trip
  // at the end of every wave; no other wave of this launch writes them)
  const float s0a = row_scale<F>(w, 2 * pc), s0b = row_scale<F>(w, min(2 * pc + 1, N - 1));
  float r0a = 0.f, r0b = 0.f;
  if constexpr (ACCUM) {
    r0a = out[2 * pc];
    r0b = out[min(2 * pc + 1, N - 1)];
  }
  __builtin_amdgcn_sched_barrier(0);
  if constexpr (NX > 0) xp.finish(K, xs);
  else stage_plain16<F>(x, K, xs);
  auto epi = [&](int p, float da, float db) {
    if (lane != 0) return;
    const int ra = 2 * p, rb = 2 * p + 1;
    da = descale<F>(da, p == p0, s0a, w, ra);
    if (ACCUM) out[ra] = da + (p == p0 ? r0a : out[ra]); else out[ra] = da;
    if (rb < N) {
      db = descale<F>(db, p == p0, s0b, w, rb);
      if (ACCUM) out[rb] = db + (p == p0 ? r0b : out[rb]); else out[rb] = db;
    }
  };
  run_pairs<F, DT, false, U, PFC>(map, epi, xs, K, npairs, p0, gridDim.x * kGemvWaves, pre);
}

// Greedy token selection fused into the lm_head (SEL): repeat penalty on the logits of
// the last `last_n` history tokens, argmax (ties -> smallest index), and the step
// finalizer (tok, history, pos) — what repeat_penalty_kernel + argmax_kernel +
// finalize_kernel (sampling.hip) do in three more launches after the lm_head.
struct HeadSel {
  const int* hist;         // token history [max_hist]
  const int* hist_len;     // device scalar
  int last_n;              // <= 256 (4 window tokens per lane)
  float penalty;           // 1 = none
  unsigned long long* slot;  // best key (ordered(logit) << 32 | ~index), 0 between launches
  unsigned int* ticket;      // finished workgroups, 0 between launches
  int* tok;                // next input token
  int* hist_w;             // history (written by the last workgroup)
  int* hist_len_w;
  int* pos;
  int max_hist;
  const uint16_t* embed;   // optional: the next step's input, resid = embed[tok] (f32)
  float* emb_out;
  int H;
};

__device__ __forceinline__ unsigned int ordered_key(float f) {
  const unsigned int u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// the lane's share of the penalty window (4 tokens per lane, -1 = none)
__device__ __forceinline__ void head_sel_window(const HeadSel& hs, int hlen, int lane, int* win) {
  const int n = min(hs.last_n, hlen), start = hlen - n;
#pragma unroll
  for (int j = 0; j < 4; ++j) win[j] = j * 64 + lane < n ? hs.hist[start + j * 64 + lane] : -1;
}

// penalty on the pair's (wave-uniform) logits — the row is one of the window's tokens, each
// token once, like the unique-token loop of repeat_penalty_kernel — and the running best key
// of the wave
__device__ __forceinline__ void head_sel_pair(const HeadSel& hs, const int* win, int ra, int rb,
                                              int N, float& da, float& db,
                                              unsigned long long& best) {
  if (hs.penalty != 1.f) {
    const bool ia = win[0] == ra || win[1] == ra || win[2] == ra || win[3] == ra;
    const bool ib = win[0] == rb || win[1] == rb || win[2] == rb || win[3] == rb;
    if (__builtin_amdgcn_ballot_w64(ia) != 0ull) da = da >= 0.f ? da / hs.penalty : da * hs.penalty;
    if (__builtin_amdgcn_ballot_w64(ib) != 0ull) db = db >= 0.f ? db / hs.penalty : db * hs.penalty;
  }
  const unsigned long long ka =
      ((unsigned long long)ordered_key(da) << 32) | (0xffffffffu - (unsigned int)ra);
  best = ka > best ? ka : best;
  if (rb < N) {
    const unsigned long long kb =
        ((unsigned long long)ordered_key(db) << 32) | (0xffffffffu - (unsigned int)rb);
    best = kb > best ? kb : best;
  }
}

// block max -> one returning 8-byte device atomic on the slot, drained before the ticket
// (atomics on both sides: the last workgroup reads the slot atomically); the last workgroup
// finalizes the step and gathers the next input row (16-bit table: what embed_kernel would
// launch for).
// Its words live in `lds`, the start of the kernel's dynamic LDS (the x row, dead after the
// pair loop; >= 64 bytes), not in static __shared__ variables: those sit in front of the
// dynamic region, and the 40 bytes they took left its base 8 bytes off a 16-byte boundary,
// which made every ds_read_b128 of x in the pair loop an unaligned (replayed) access.
template <int DT>
__device__ __forceinline__ void head_sel_tail(const HeadSel& hs, unsigned long long best,
                                              void* lds) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  unsigned long long* red = reinterpret_cast<unsigned long long*>(lds);  // [kGemvWaves]
  int& is_last = reinterpret_cast<int*>(lds)[2 * kGemvWaves];
  int& sel_tok = reinterpret_cast<int*>(lds)[2 * kGemvWaves + 1];
  __syncthreads();  // every wave has read its last x
  if (lane == 0) red[wave] = best;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long b = red[0];
#pragma unroll
    for (int i = 1; i < kGemvWaves; ++i) b = red[i] > b ? red[i] : b;
    const unsigned long long old =
        __hip_atomic_fetch_max(hs.slot, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::"v"((unsigned int)old) : "memory");
    const unsigned int t =
        __hip_atomic_fetch_add(hs.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    is_last = t == gridDim.x - 1;
  }
  __syncthreads();
  if (is_last) {  // block-uniform
    if (threadIdx.x == 0) {
      const unsigned long long key =
          __hip_atomic_fetch_max(hs.slot, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const int t = (int)(0xffffffffu - (unsigned int)(key & 0xffffffffull));
      *hs.tok = t;
      const int len = *hs.hist_len_w;
      if (len < hs.max_hist) { hs.hist_w[len] = t; *hs.hist_len_w = len + 1; }
      *hs.pos += 1;
      // re-arm for the next launch (the kernel boundary orders these for it)
      __hip_atomic_store(hs.slot, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(hs.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      sel_tok = t;
    }
    if (hs.embed != nullptr) {
      // every other workgroup has finished reading resid (their tickets preceded this one)
      __syncthreads();
      const uint16_t* row = hs.embed + (size_t)sel_tok * hs.H;
      for (int i = threadIdx.x * 8; i < hs.H; i += kGemvThreads * 8) {
        float f[8];
        unpack8<DT>(*reinterpret_cast<const uint4*>(row + i), f);
        *reinterpret_cast<float4*>(hs.emb_out + i) = make_float4(f[0], f[1], f[2], f[3]);
        *reinterpret_cast<float4*>(hs.emb_out + i + 4) = make_float4(f[4], f[5], f[6], f[7]);
      }
    }
  }
}

// RMSNorm(f32 row) then f32 output: the lm_head (SEL: + greedy selection, see HeadSel; the
// next input row comes from the 16-bit embedding table whatever the head's format).
template <class F, int DT, int U, int PFC, int NX, bool SEL>
__global__ __launch_bounds__(kGemvThreads) void gemv_norm_f32_kernel(
    const float* __restrict__ resid, const uint16_t* __restrict__ norm_w, float eps,
    const typename F::Mat w, int K, int N, float* __restrict__ out, HeadSel hs) {
  extern __shared__ float xs[];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int npairs = (N + 1) >> 1;
  const int p0 = blockIdx.x * kGemvWaves + wave;
  auto map = [&](int p) { return F::rows(w, (size_t)(2 * p), w, (size_t)min(2 * p + 1, N - 1), K); };
  // SEL: the history length is requested ahead of the x prologue (one load in front of
  // it), the window itself after it (queued behind the first weight rows; first needed
  // by the first pair's epilogue)
  int hlen = 0;
  if constexpr (SEL) hlen = hs.penalty != 1.f ? *hs.hist_len : 0;
  Regs<F, PFC> pre;
  NormPre<F, DT, NX> xp;
  const int pc = p0 < npairs ? p0 : npairs - 1;
  const typename F::Rows r0 = map(pc);
  keep_rows<F, PFC>(r0, pre);
  if constexpr (NX > 0) xp.load(resid, norm_w, K);
  __builtin_amdgcn_sched_barrier(0);  // x loads strictly before the weights (in-order vmcnt)
  if (NX > 0 || (PFC > 0 && p0 < npairs)) prefetch_rows<F, PFC>(r0, pre);  // NX: exact vmcnt
  // the first pair's row scales, requested now (one address per wave: every lane holds
  // the value, which the SEL ballot and key need wave-wide)
  const float s0a = row_scale<F>(w, 2 * pc), s0b = row_scale<F>(w, min(2 * pc + 1, N - 1));
  __builtin_amdgcn_sched_barrier(0);
  if constexpr (NX > 0) xp.finish(eps, K, xs);
  else stage_rmsnorm<F, DT>(resid, norm_w, eps, K, xs);
  int win[4] = {-1, -1, -1, -1};
  if constexpr (SEL) head_sel_window(hs, hlen, lane, win);
  unsigned long long best = 0ull;
  auto epi = [&](int p, float da, float db) {
    const int ra = 2 * p, rb = 2 * p + 1;
    // the row scales first: everything below sees the logits
    da = descale<F>(da, p == p0, s0a, w, ra);
    db = descale<F>(db, p == p0, s0b, w, min(rb, N - 1));
    if constexpr (SEL) head_sel_pair(hs, win, ra, rb, N, da, db, best);
    if (lane != 0) return;
    out[ra] = da;
    if (rb < N) out[rb] = db;
  };
  run_pairs<F, DT, true, U, PFC>(map, epi, xs, K, npairs, p0, gridDim.x * kGemvWaves, pre);
  if constexpr (SEL) head_sel_tail<DT>(hs, best, xs);
}

static inline int grid_for(int npairs, int max_blocks) {
  int g = (npairs + kGemvWaves - 1) / kGemvWaves;
  return g < max_blocks ? g : max_blocks;
}

}  // namespace cake

using namespace cake;

// ---------------------------------------------------------------------------
// Launchers: one per kernel kind, shared by the formats.  The cake_* entry points
// (gemv*.hip) cast their pointers into F::Mat handles and call these.
// ---------------------------------------------------------------------------

#define DISPATCH_DT(dt, ...)                       \
  do {                                             \
    if ((dt) == kBF16) { constexpr int DT = kBF16; __VA_ARGS__; } \
    else if ((dt) == kF16) { constexpr int DT = kF16; __VA_ARGS__; } \
    else return (int)hipErrorInvalidValue;         \
  } while (0)
// the launchers' form: a format of bf16 rows alone (kBf16Only) has no f16 kernels
#define DISPATCH_DT_F(F, dt, ...)                  \
  do {                                             \
    if constexpr (Bf16Only<F>::value) {            \
      if ((dt) == kBF16) { constexpr int DT = kBF16; __VA_ARGS__; } \
      else return (int)hipErrorInvalidValue;       \
    } else DISPATCH_DT(dt, __VA_ARGS__);           \
  } while (0)

// Expand BODY for the run-time (U, PF) choice among those format F instantiates: t.U is one
// of F::kU (gemv_set_tuning refuses any other), the prefetch depth is what F::prefetch makes
// of t.PF for a row of K values (one of F::kPF, or 0).
#define CAKE_TUNE_U(F, PFCV, ...)                                                              \
  if (t.U == F::kU[0]) { constexpr int U = F::kU[0]; constexpr int PF = PFCV; __VA_ARGS__; }      \
  else if (t.U == F::kU[1]) { constexpr int U = F::kU[1]; constexpr int PF = PFCV; __VA_ARGS__; } \
  else { constexpr int U = F::kU[2]; constexpr int PF = PFCV; __VA_ARGS__; }
#define DISPATCH_TUNE(F, t, K, ...)                                                  \
  do {                                                                               \
    const int pfc_ = F::prefetch((t).PF, K);                                         \
    if (pfc_ == F::kPF[0]) { CAKE_TUNE_U(F, F::kPF[0], __VA_ARGS__) }                \
    else if (pfc_ == F::kPF[1]) { CAKE_TUNE_U(F, F::kPF[1], __VA_ARGS__) }           \
    else { CAKE_TUNE_U(F, 0, __VA_ARGS__) }                                          \
  } while (0)
// NX: split x prologue (only with a weight prefetch): RMSNorm rows K <= 1024 NX,
// 16-bit rows K <= 2048 NX (guarded tails: the TP shards' K); larger K use the
// plain prologue (NX = 0).
#define CAKE_NX_NORM(K, ...)                                                         \
  if constexpr (PF > 0) {                                                            \
    if ((K) <= 4096) { constexpr int NX = 4; __VA_ARGS__; }                          \
    else if ((K) <= 8192) { constexpr int NX = 8; __VA_ARGS__; }                     \
    else { constexpr int NX = 0; __VA_ARGS__; }                                      \
  } else { constexpr int NX = 0; __VA_ARGS__; }
#define CAKE_NX_X16(K, ...)                                                          \
  if constexpr (PF > 0) {                                                            \
    if ((K) <= 2048) { constexpr int NX = 1; __VA_ARGS__; }                          \
    else if ((K) <= 4096) { constexpr int NX = 2; __VA_ARGS__; }                     \
    else if ((K) <= 8192) { constexpr int NX = 4; __VA_ARGS__; }                     \
    else if ((K) <= 14336) { constexpr int NX = 7; __VA_ARGS__; }                    \
    else if ((K) <= 28672) { constexpr int NX = 14; __VA_ARGS__; }                   \
    else { constexpr int NX = 0; __VA_ARGS__; }                                      \
  } else { constexpr int NX = 0; __VA_ARGS__; }

// K must be whole chunks; kStrict: at least one, and n (the output rows) at least 1
template <class F> static inline bool bad_shape(int K, int n) {
  return K % (1 << F::kLog2) != 0 || (F::kStrict && (K < (1 << F::kLog2) || n < 1));
}
template <class F> static inline size_t x32_lds_bytes(int K) {
  return (size_t)((K + F::kPad32 - 1) / F::kPad32 * F::kPad32) * sizeof(float);
}
template <class F> static inline size_t x16_lds_bytes(int K) {
  return (size_t)((K + F::kPad16 - 1) / F::kPad16 * F::kPad16) * sizeof(uint16_t);
}

template <class F> static int gemv_set_tuning(int kind, int U, int prefetch, int max_blocks) {
  if (kind < 0 || kind >= F::kKinds || (U != F::kU[0] && U != F::kU[1] && U != F::kU[2]) ||
      max_blocks < 1 || (prefetch != 0 && prefetch != F::kPF[0] && prefetch != F::kPF[1]))
    return (int)hipErrorInvalidValue;
  g_tune[F::kFmt][kind] = GemvTune{U, prefetch, max_blocks};
  return 0;
}

template <class F> static int gemv_get_tuning(int kind, int* out3) {
  if (kind < 0 || kind >= F::kKinds || !out3) return (int)hipErrorInvalidValue;
  const GemvTune t = g_tune[F::kFmt][kind];
  out3[0] = t.U;
  out3[1] = t.PF;
  out3[2] = t.MB;
  return 0;
}

// kv_fmt (common.h KvFmt): 0 = 16-bit cache rows, 1 = kcache / vcache hold one e4m3fn code
// per element (quant_kv_fp8 of the f32 roped K / f32 V), 2 = those codes' values as 16 bits
template <class F> static int launch_qkv(int dt, const QkvArgs<F>& a, hipStream_t st) {
  if (bad_shape<F>(a.K, a.nh < a.nkv ? a.nh : a.nkv) || a.hd % 2 || a.kv_fmt < 0 || a.kv_fmt > 2)
    return (int)hipErrorInvalidValue;
  const int K = a.K, npairs = (a.nh + 2 * a.nkv) * (a.hd / 2);
  const size_t lds = x32_lds_bytes<F>(K);
  const GemvTune t = g_tune[F::kFmt][kQkv];
  DISPATCH_DT_F(F, dt, DISPATCH_TUNE(F, t, K, CAKE_NX_NORM(K, hipLaunchKernelGGL((qkv_rope_kernel<F, DT, U, PF, NX>),
                                                         dim3(grid_for(npairs, t.MB)),
                                                         dim3(kGemvThreads), lds, st, a))));
  return (int)hipGetLastError();
}

template <class F>
static int launch_swiglu(int dt, const float* resid, const void* norm_w, float eps,
                         typename F::Mat wg, typename F::Mat wu, int K, int I, void* act,
                         hipStream_t st) {
  if (bad_shape<F>(K, I)) return (int)hipErrorInvalidValue;
  const size_t lds = x32_lds_bytes<F>(K);
  const GemvTune t = g_tune[F::kFmt][kSwiglu];
  // at least one block per 28 rows (7 row pairs per wave): 70B's I = 28672 runs 1024
  // blocks (+0.7 %, profiles/r2_decode_gemv_tuning_70b.jsonl), 8B's 14336 the tuned cap
  const int mb = t.MB > (I + 27) / 28 ? t.MB : (I + 27) / 28;
  DISPATCH_DT_F(F, dt, DISPATCH_TUNE(F, t, K, CAKE_NX_NORM(K, hipLaunchKernelGGL((swiglu_kernel<F, DT, U, PF, NX>),
                                                         dim3(grid_for(I, mb)), dim3(kGemvThreads),
                                                         lds, st, resid, (const uint16_t*)norm_w, eps,
                                                         wg, wu, K, I, (uint16_t*)act))));
  return (int)hipGetLastError();
}

template <class F>
static int launch_x16(int dt, const void* x, typename F::Mat w, int K, int N, float* out,
                      int accumulate, hipStream_t st) {
  if (bad_shape<F>(K, N)) return (int)hipErrorInvalidValue;
  const size_t lds = x16_lds_bytes<F>(K);
  const GemvTune t = g_tune[F::kFmt][F::kKinds > kX16S && K <= 8192 ? kX16S : kX16];
  const int g = grid_for((N + 1) / 2, t.MB);
  if (accumulate) {
    DISPATCH_DT_F(F, dt, DISPATCH_TUNE(F, t, K, CAKE_NX_X16(K, hipLaunchKernelGGL((gemv_x16_kernel<F, DT, U, PF, NX, true>),
                                                          dim3(g), dim3(kGemvThreads), lds, st,
                                                          (const uint16_t*)x, w, K, N, out))));
  } else {
    DISPATCH_DT_F(F, dt, DISPATCH_TUNE(F, t, K, CAKE_NX_X16(K, hipLaunchKernelGGL((gemv_x16_kernel<F, DT, U, PF, NX, false>),
                                                          dim3(g), dim3(kGemvThreads), lds, st,
                                                          (const uint16_t*)x, w, K, N, out))));
  }
  return (int)hipGetLastError();
}

template <class F, bool SEL>
static int launch_norm_f32(int dt, const float* resid, const void* norm_w, float eps,
                           typename F::Mat w, int K, int N, float* out, const HeadSel& hs,
                           hipStream_t st) {
  if (bad_shape<F>(K, N)) return (int)hipErrorInvalidValue;
  // SEL: at least the 64 bytes head_sel_tail keeps its words in (a 16-bit K of 8)
  const size_t lds = SEL && x32_lds_bytes<F>(K) < 64 ? 64 : x32_lds_bytes<F>(K);
  const GemvTune t = g_tune[F::kFmt][kNormF32];
  DISPATCH_DT_F(F, dt, DISPATCH_TUNE(F, t, K, CAKE_NX_NORM(K, hipLaunchKernelGGL((gemv_norm_f32_kernel<F, DT, U, PF, NX, SEL>),
                                                         dim3(grid_for((N + 1) / 2, t.MB)),
                                                         dim3(kGemvThreads), lds, st, resid,
                                                         (const uint16_t*)norm_w, eps, w, K, N,
                                                         out, hs))));
  return (int)hipGetLastError();
}

// lm_head + repeat penalty + argmax + step finalizer in one launch (greedy decode);
// with `embed`, also the next step's input emb_out[K] = embed[tok] (f32).  slot (u64)
// and ticket (u32) must be zero before the first launch; the kernel re-arms them.
// last_n <= 256.
template <class F>
static int launch_head_select(int dt, const float* resid, const void* norm_w, float eps,
                              typename F::Mat w, int K, int N, float* out, int* hist,
                              int* hist_len, int last_n, float penalty, unsigned long long* slot,
                              unsigned int* ticket, int* tok, int* pos, int max_hist,
                              const void* embed, float* emb_out, hipStream_t st) {
  if (last_n < 0 || last_n > kHeadSelectMaxLastN || !(penalty > 0.f) || slot == nullptr ||
      ticket == nullptr || (embed != nullptr && emb_out == nullptr))
    return (int)hipErrorInvalidValue;
  const HeadSel hs{hist, hist_len, last_n, penalty, slot, ticket, tok, hist, hist_len, pos,
                   max_hist, (const uint16_t*)embed, emb_out, K};
  return launch_norm_f32<F, true>(dt, resid, norm_w, eps, w, K, N, out, hs, st);
}
