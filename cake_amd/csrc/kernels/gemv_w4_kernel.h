// Decode GEMV kernels over MXFP4 weight-only projections: the 4-bit twins of
// qkv_rope_kernel / swiglu_kernel / gemv_x16_kernel / gemv_norm_f32_kernel (gemv_kernel.h),
// shared by gemv_w4.hip, gemv_w4_mlp.hip, gemv_w4_x16.hip and gemv_w4_head.hip (one launcher
// per translation unit so the instantiations compile in parallel).
//
// Format (quant_mxfp4.hip writes it): w4[N, K/2] two e2m1 codes per byte (k even in the low
// nibble), e8[N, K/32] one e8m0 scale byte per 32 consecutive k,
// W[n, k] = 2^(e8[n, k/32] - 127) * e2m1(code).  K % 32 == 0.
//
// Same structure as the 16-bit and fp8 kernels: one wave per pair of rows, the x prologue
// loads issued before the wave's first weight rows, the first pair prefetched in registers,
// 16-byte non-temporal loads, f32 accumulation, wave_sum reductions, compile-time register
// indices.  A lane's 16-byte chunk now carries 32 k values — exactly one scale block — so
// each chunk comes with one scale byte per row (a wave's 64 chunks read 64 consecutive
// bytes of e8), requested together with the chunk.  The convert applies the block scale
// (v_cvt_scalef32_pk_f32_fp4: two codes and the scale per instruction), so the accumulators
// hold scaled products and the epilogues are those of the 16-bit kernels.
#pragma once
#include "gemv_kernel.h"
#include "mxfp4.h"

namespace cake {

// The x row is kept in LDS in a permuted order, as x32_perm (gemv_w8_kernel.h) does for the
// fp8 kernels.  A lane's chunk is 32 consecutive values: 128 bytes of f32 or 64 bytes of
// 16-bit.  ds_read_b128 serves 16 lanes at a time over a 256-byte bank row, so a 128-byte
// lane stride is an 8-way conflict and a 64-byte one 4-way.  Within every block of 64
// chunks (2048 values) the j-th 16-byte word of chunk l sits at word index j * 64 + l
// (8 words per chunk in f32, 4 in 16-bit): each read of a lane is then contiguous across
// the wave.  LDS holds K rounded up to 2048 values.
__device__ __forceinline__ int x32_perm4(int i) {  // i % 4 == 0: index of a float4's first float
  return (i & ~2047) | (((i >> 2) & 7) << 8) | (((i & 2047) >> 5) << 2);
}
__device__ __forceinline__ int x16_perm4(int i) {  // i % 8 == 0: index of a uint4's first value
  return (i & ~2047) | (((i >> 3) & 3) << 9) | (((i & 2047) >> 5) << 3);
}
static inline size_t x32_lds_bytes4(int K) { return (size_t)((K + 2047) & ~2047) * sizeof(float); }
static inline size_t x16_lds_bytes4(int K) { return (size_t)((K + 2047) & ~2047) * sizeof(uint16_t); }

template <int DT>
__device__ __forceinline__ void stage_rmsnorm_perm4(const float* __restrict__ x,
                                                    const uint16_t* __restrict__ w, float eps,
                                                    int K, float* xs) {
  __shared__ float red[16];
  float ss = 0.f;
  for (int i = threadIdx.x * 4; i < K; i += kGemvThreads * 4) {
    const float4 v = *reinterpret_cast<const float4*>(x + i);
    *reinterpret_cast<float4*>(xs + x32_perm4(i)) = v;
    ss += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
  }
  ss = block_sum(ss, red);
  const float r = rsqrtf(ss / (float)K + eps);
  for (int i = threadIdx.x * 4; i < K; i += kGemvThreads * 4) {
    float4 v = *reinterpret_cast<float4*>(xs + x32_perm4(i));
    const uint2 wv = *reinterpret_cast<const uint2*>(w + i);
    v.x *= r * to_f32<DT>((uint16_t)(wv.x & 0xffff));
    v.y *= r * to_f32<DT>((uint16_t)(wv.x >> 16));
    v.z *= r * to_f32<DT>((uint16_t)(wv.y & 0xffff));
    v.w *= r * to_f32<DT>((uint16_t)(wv.y >> 16));
    *reinterpret_cast<float4*>(xs + x32_perm4(i)) = v;
  }
  __syncthreads();
}

// NormPre (gemv_kernel.h) with the permuted LDS image
template <int DT, int NX> struct NormPreW4 : NormPre<DT, NX> {
  __device__ __forceinline__ void finish(float eps, int K, float* xs) {
    __shared__ float red[16];
    float ss = 0.f;
#pragma unroll
    for (int j = 0; j < NX; ++j) {
      const float4 v = this->x[j];
      ss += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
    }
    ss = block_sum(ss, red);
    const float r = rsqrtf(ss / (float)K + eps);
#pragma unroll
    for (int j = 0; j < NX; ++j) {
      const int i = (j * kGemvThreads + threadIdx.x) * 4;
      float4 v = this->x[j];
      const uint2 wv = this->w[j];
      v.x *= r * to_f32<DT>((uint16_t)(wv.x & 0xffff));
      v.y *= r * to_f32<DT>((uint16_t)(wv.x >> 16));
      v.z *= r * to_f32<DT>((uint16_t)(wv.y & 0xffff));
      v.w *= r * to_f32<DT>((uint16_t)(wv.y >> 16));
      if (i < K) *reinterpret_cast<float4*>(xs + x32_perm4(i)) = v;
    }
    __syncthreads();
  }
};

__device__ __forceinline__ void stage_plain16_perm4(const uint16_t* __restrict__ x, int K,
                                                    uint16_t* xs) {
  for (int i = threadIdx.x * 8; i < K; i += kGemvThreads * 8)
    *reinterpret_cast<uint4*>(xs + x16_perm4(i)) = *reinterpret_cast<const uint4*>(x + i);
  __syncthreads();
}

// Plain16Pre (gemv_kernel.h) with the permuted LDS image
template <int NX> struct Plain16PreW4 : Plain16Pre<NX> {
  __device__ __forceinline__ void finish(int K, uint16_t* xs) {
#pragma unroll
    for (int j = 0; j < NX; ++j) {
      const int i = (j * kGemvThreads + threadIdx.x) * 8;
      if (i < K) *reinterpret_cast<uint4*>(xs + x16_perm4(i)) = this->v[j];
    }
    __syncthreads();
  }
};

// 8 x values of a chunk: those of code dword D (k = 8 D .. 8 D + 7)
template <int DT, bool XF32, int D>
__device__ __forceinline__ void load_x8_w4(const void* xs, int chunk, float* o) {
  if constexpr (XF32) {
    const float4* p = reinterpret_cast<const float4*>(xs) + ((chunk >> 6) << 9) + (chunk & 63);
    const float4 a = p[(2 * D) * 64], b = p[(2 * D + 1) * 64];
    o[0] = a.x; o[1] = a.y; o[2] = a.z; o[3] = a.w;
    o[4] = b.x; o[5] = b.y; o[6] = b.z; o[7] = b.w;
  } else {
    const uint4* p = reinterpret_cast<const uint4*>(xs) + ((chunk >> 6) << 8) + (chunk & 63);
    unpack8<DT>(p[D * 64], o);
  }
}

template <int D>
__device__ __forceinline__ void fma_dword_w4(const float* xv, uint32_t wa, uint32_t wb, float sa,
                                             float sb, f32x2_t& acc_a, f32x2_t& acc_b) {
  const f32x2_t x01 = {xv[0], xv[1]}, x23 = {xv[2], xv[3]};
  const f32x2_t x45 = {xv[4], xv[5]}, x67 = {xv[6], xv[7]};
  acc_a = __builtin_elementwise_fma(fp4x2_to_f32<0>(wa, sa), x01, acc_a);
  acc_b = __builtin_elementwise_fma(fp4x2_to_f32<0>(wb, sb), x01, acc_b);
  acc_a = __builtin_elementwise_fma(fp4x2_to_f32<1>(wa, sa), x23, acc_a);
  acc_b = __builtin_elementwise_fma(fp4x2_to_f32<1>(wb, sb), x23, acc_b);
  acc_a = __builtin_elementwise_fma(fp4x2_to_f32<2>(wa, sa), x45, acc_a);
  acc_b = __builtin_elementwise_fma(fp4x2_to_f32<2>(wb, sb), x45, acc_b);
  acc_a = __builtin_elementwise_fma(fp4x2_to_f32<3>(wa, sa), x67, acc_a);
  acc_b = __builtin_elementwise_fma(fp4x2_to_f32<3>(wb, sb), x67, acc_b);
}

// one chunk of both rows: 32 k values, ea / eb the chunk's scale bytes
template <int DT, bool XF32>
__device__ __forceinline__ void fma_chunk_w4(const void* xs, int chunk, const uint4 va,
                                             const uint4 vb, uint32_t ea, uint32_t eb,
                                             f32x2_t& acc_a, f32x2_t& acc_b) {
  const float sa = e8m0_to_f32(ea), sb = e8m0_to_f32(eb);
  float xv[8];
  load_x8_w4<DT, XF32, 0>(xs, chunk, xv);
  fma_dword_w4<0>(xv, va.x, vb.x, sa, sb, acc_a, acc_b);
  load_x8_w4<DT, XF32, 1>(xs, chunk, xv);
  fma_dword_w4<1>(xv, va.y, vb.y, sa, sb, acc_a, acc_b);
  load_x8_w4<DT, XF32, 2>(xs, chunk, xv);
  fma_dword_w4<2>(xv, va.z, vb.z, sa, sb, acc_a, acc_b);
  load_x8_w4<DT, XF32, 3>(xs, chunk, xv);
  fma_dword_w4<3>(xv, va.w, vb.w, sa, sb, acc_a, acc_b);
}

// the code and scale rows of a pair
struct RowsW4 {
  const uint8_t *wa, *wb;  // [K/2] codes
  const uint8_t *ea, *eb;  // [K/32] scale bytes
};

// prefetch registers: PFC chunks per row per lane and their scale bytes
template <int N> struct RegsW4 { uint4 a[N], b[N]; uint32_t ea[N], eb[N]; };
template <> struct RegsW4<0> { uint4 a[1], b[1]; uint32_t ea[1], eb[1]; };

// accumulate chunks [c_start, nch) of the pair (c_start a multiple of 64)
template <int DT, bool XF32, int U>
__device__ __forceinline__ void dot_range_w4(const RowsW4& r, const void* xs, int nch, int c_start,
                                             f32x2_t& acc_a, f32x2_t& acc_b) {
  const int lane = threadIdx.x & 63;
  const uint4* a4 = reinterpret_cast<const uint4*>(r.wa);
  const uint4* b4 = reinterpret_cast<const uint4*>(r.wb);
  const int full = c_start + ((nch - c_start) / (64 * U)) * (64 * U);
  for (int c0 = c_start; c0 < full; c0 += 64 * U) {
    uint4 va[U], vb[U];
    uint32_t ea[U], eb[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      va[u] = ld_nt16(a4 + c0 + u * 64 + lane);
      vb[u] = ld_nt16(b4 + c0 + u * 64 + lane);
      ea[u] = r.ea[c0 + u * 64 + lane];
      eb[u] = r.eb[c0 + u * 64 + lane];
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
      fma_chunk_w4<DT, XF32>(xs, c0 + u * 64 + lane, va[u], vb[u], ea[u], eb[u], acc_a, acc_b);
  }
  // the tail: lanes past nch have no chunk (K / 32 < 64: most of the wave)
  for (int c = full + lane; c < nch; c += 64)
    fma_chunk_w4<DT, XF32>(xs, c, a4[c], b4[c], r.ea[c], r.eb[c], acc_a, acc_b);
}

// issue the first PFC chunks of the pair (nch >= 64 PFC)
template <int PFC>
__device__ __forceinline__ void prefetch_rows_w4(const RowsW4& r, RegsW4<PFC>& g) {
  if constexpr (PFC > 0) {
    const int lane = threadIdx.x & 63;
    const uint4* a4 = reinterpret_cast<const uint4*>(r.wa);
    const uint4* b4 = reinterpret_cast<const uint4*>(r.wb);
#pragma unroll
    for (int c = 0; c < PFC; ++c) {
      g.a[c] = ld_nt16(a4 + c * 64 + lane);
      g.b[c] = ld_nt16(b4 + c * 64 + lane);
      g.ea[c] = r.ea[c * 64 + lane];
      g.eb[c] = r.eb[c * 64 + lane];
    }
  }
}

// run_pairs (gemv_kernel.h) over MXFP4 rows; epi gets the scaled dot products
template <int DT, bool XF32, int U, int PFC, class Map, class Epi>
__device__ __forceinline__ void run_pairs_w4(const Map& map, const Epi& epi, const void* xs, int K,
                                             int npairs, int p0, int stride,
                                             const RegsW4<PFC>& pre) {
  const int nch = K >> 5;
  int p = p0;
  if constexpr (PFC > 0) {
    // unconditional, as in run_pairs: an idle wave works on a clamped pair and drops it
    const RowsW4 r = map(p < npairs ? p : npairs - 1);
    const int lane = threadIdx.x & 63;
    f32x2_t aa = {0.f, 0.f}, ab = {0.f, 0.f};
#pragma unroll
    for (int c = 0; c < PFC; ++c)
      fma_chunk_w4<DT, XF32>(xs, c * 64 + lane, pre.a[c], pre.b[c], pre.ea[c], pre.eb[c], aa, ab);
    dot_range_w4<DT, XF32, U>(r, xs, nch, PFC * 64, aa, ab);
    const float sa = wave_sum(aa.x + aa.y), sb = wave_sum(ab.x + ab.y);
    if (p < npairs) epi(p, sa, sb);
    p += stride;
  }
  for (; p < npairs; p += stride) {
    const RowsW4 r = map(p);
    f32x2_t aa = {0.f, 0.f}, ab = {0.f, 0.f};
    dot_range_w4<DT, XF32, U>(r, xs, nch, 0, aa, ab);
    epi(p, wave_sum(aa.x + aa.y), wave_sum(ab.x + ab.y));
  }
}

// ---------------------------------------------------------------------------
// QKV + RoPE + KV-cache write
// ---------------------------------------------------------------------------
struct QkvW4Args {
  const float* resid;      // [K] f32
  const uint16_t* norm_w;  // [K]
  float eps;
  const uint8_t* wq;  // [nh*hd, K/2] codes
  const uint8_t* wk;  // [nkv*hd, K/2]
  const uint8_t* wv;  // [nkv*hd, K/2]
  const uint8_t* eq;  // [nh*hd, K/32] scale bytes
  const uint8_t* ek;  // [nkv*hd, K/32]
  const uint8_t* ev;  // [nkv*hd, K/32]
  int K, nh, nkv, hd;
  const float* inv_freq;  // [hd/2]
  const int* pos;         // device scalar: position of this token
  float* q_out;           // [nh*hd] f32 (roped)
  uint16_t* kcache;       // [nkv][S][hd] (this layer)
  uint16_t* vcache;
  int S;
  int kv_fmt;             // KvFmt of the cache (common.h); 1: kcache / vcache hold bytes
};

template <int DT, int U, int PFC, int NX>
__global__ __launch_bounds__(kGemvThreads) void qkv_rope_w4_kernel(QkvW4Args a) {
  extern __shared__ float xs[];
  const int half = a.hd >> 1;
  const int npairs = (a.nh + 2 * a.nkv) * half;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int p0 = blockIdx.x * kGemvWaves + wave;
  // bases selected by address arithmetic, not a pointer select (see qkv_rope_kernel)
  const uint8_t* wq = a.wq;
  const uint8_t* eq = a.eq;
  const ptrdiff_t dk = a.wk - a.wq, dv = a.wv - a.wq;
  const ptrdiff_t dek = a.ek - a.eq, dev = a.ev - a.eq;
  const int nh = a.nh, nqk = a.nh + a.nkv, hd = a.hd;
  const size_t rowb = (size_t)a.K >> 1, rowe = (size_t)a.K >> 5;
  // kind 0 = q, 1 = k, 2 = v; ra = the pair's first row inside its matrix
  auto where = [=](int p, int& kind, int& head, size_t& ra) {
    const int slot = p / half;
    const bool isq = slot < nh, isk = !isq && slot < nqk;
    kind = isq ? 0 : (isk ? 1 : 2);
    head = slot - (isq ? 0 : (isk ? nh : nqk));
    ra = (size_t)head * hd + (p - slot * half);
  };
  auto map = [=](int p) {
    int kind, head;
    size_t ra;
    where(p, kind, head, ra);
    const uint8_t* wb = wq + (kind == 0 ? 0 : (kind == 1 ? dk : dv));
    const uint8_t* eb = eq + (kind == 0 ? 0 : (kind == 1 ? dek : dev));
    return RowsW4{wb + ra * rowb, wb + (ra + half) * rowb, eb + ra * rowe, eb + (ra + half) * rowe};
  };
  RegsW4<PFC> pre;
  NormPreW4<DT, NX> xp;
  const int pc = p0 < npairs ? p0 : npairs - 1;
  const RowsW4 r0 = map(pc);  // rows first: their address math may load (kernarg select)
  if constexpr (NX > 0) xp.load(a.resid, a.norm_w, a.K);
  __builtin_amdgcn_sched_barrier(0);  // x loads strictly before the weights (in-order vmcnt)
  if (NX > 0 || (PFC > 0 && p0 < npairs)) prefetch_rows_w4<PFC>(r0, pre);  // NX: exact vmcnt
  // the RoPE frequency of the wave's first pair, requested now
  const float f0 = a.inv_freq[pc - (pc / half) * half];
  __builtin_amdgcn_sched_barrier(0);
  if constexpr (NX > 0) xp.finish(a.eps, a.K, xs);
  else stage_rmsnorm_perm4<DT>(a.resid, a.norm_w, a.eps, a.K, xs);
  const int pos = *a.pos;
  auto epi = [&](int p, float da, float db) {
    if (lane != 0) return;
    int kind, head;
    size_t ra;
    where(p, kind, head, ra);
    const int i = p - (p / half) * half;
    float oa = da, ob = db;
    if (kind < 2) {
      float s, c;
      sincosf((float)pos * (p == p0 ? f0 : a.inv_freq[i]), &s, &c);
      oa = da * c - db * s;
      ob = da * s + db * c;
    }
    if (kind == 0) {
      a.q_out[ra] = oa;
      a.q_out[ra + half] = ob;
    } else {
      uint16_t* cache = kind == 1 ? a.kcache : a.vcache;
      const size_t off = ((size_t)head * a.S + pos) * a.hd + i;
      kv_store_pair<DT>(cache, off, half, oa, ob, a.kv_fmt);
    }
  };
  run_pairs_w4<DT, true, U, PFC>(map, epi, xs, a.K, npairs, p0, gridDim.x * kGemvWaves, pre);
}

// ---------------------------------------------------------------------------
// RMSNorm + gate/up + SiLU*mul
// ---------------------------------------------------------------------------
template <int DT, int U, int PFC, int NX>
__global__ __launch_bounds__(kGemvThreads) void swiglu_w4_kernel(
    const float* __restrict__ resid, const uint16_t* __restrict__ norm_w, float eps,
    const uint8_t* __restrict__ wg, const uint8_t* __restrict__ wu,
    const uint8_t* __restrict__ eg, const uint8_t* __restrict__ eu, int K, int I,
    uint16_t* __restrict__ act) {
  extern __shared__ float xs[];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int j0 = blockIdx.x * kGemvWaves + wave;
  const size_t rowb = (size_t)K >> 1, rowe = (size_t)K >> 5;
  auto map = [&](int j) {
    return RowsW4{wg + (size_t)j * rowb, wu + (size_t)j * rowb, eg + (size_t)j * rowe,
                  eu + (size_t)j * rowe};
  };
  RegsW4<PFC> pre;
  NormPreW4<DT, NX> xp;
  const RowsW4 r0 = map(j0 < I ? j0 : I - 1);
  if constexpr (NX > 0) xp.load(resid, norm_w, K);
  __builtin_amdgcn_sched_barrier(0);  // x loads strictly before the weights (in-order vmcnt)
  // NX: unconditional (an idle wave re-reads the last row), so the vmcnt is exact
  if (NX > 0 || (PFC > 0 && j0 < I)) prefetch_rows_w4<PFC>(r0, pre);
  __builtin_amdgcn_sched_barrier(0);
  if constexpr (NX > 0) xp.finish(eps, K, xs);
  else stage_rmsnorm_perm4<DT>(resid, norm_w, eps, K, xs);
  auto epi = [&](int j, float g, float u) {
    if (lane == 0) act[j] = from_f32<DT>(silu(g) * u);
  };
  run_pairs_w4<DT, true, U, PFC>(map, epi, xs, K, I, j0, gridDim.x * kGemvWaves, pre);
}

// ---------------------------------------------------------------------------
// out (+)= W x   with 16-bit x: o_proj / down_proj
// ---------------------------------------------------------------------------
template <int DT, int U, int PFC, int NX, bool ACCUM>
__global__ __launch_bounds__(kGemvThreads) void gemv_x16_w4_kernel(
    const uint16_t* __restrict__ x, const uint8_t* __restrict__ w, const uint8_t* __restrict__ e8,
    int K, int N, float* __restrict__ out) {
  extern __shared__ float smem[];
  uint16_t* xs = reinterpret_cast<uint16_t*>(smem);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int npairs = (N + 1) >> 1;
  const int p0 = blockIdx.x * kGemvWaves + wave;
  const size_t rowb = (size_t)K >> 1, rowe = (size_t)K >> 5;
  auto map = [&](int p) {
    const size_t ra = (size_t)(2 * p), rb = (size_t)min(2 * p + 1, N - 1);
    return RowsW4{w + ra * rowb, w + rb * rowb, e8 + ra * rowe, e8 + rb * rowe};
  };
  RegsW4<PFC> pre;
  Plain16PreW4<NX> xp;
  const int pc = p0 < npairs ? p0 : npairs - 1;
  const RowsW4 r0 = map(pc);
  if constexpr (NX > 0) xp.load(x, K);
  __builtin_amdgcn_sched_barrier(0);  // x loads strictly before the weights (in-order vmcnt)
  if (NX > 0 || (PFC > 0 && p0 < npairs)) prefetch_rows_w4<PFC>(r0, pre);  // NX: exact vmcnt
  // ACCUM: the residual words of the wave's first pair, requested now (no other wave of
  // this launch writes them)
  float r0a = 0.f, r0b = 0.f;
  if constexpr (ACCUM) {
    r0a = out[2 * pc];
    r0b = out[min(2 * pc + 1, N - 1)];
  }
  __builtin_amdgcn_sched_barrier(0);
  if constexpr (NX > 0) xp.finish(K, xs);
  else stage_plain16_perm4(x, K, xs);
  auto epi = [&](int p, float da, float db) {
    if (lane != 0) return;
    const int ra = 2 * p, rb = 2 * p + 1;
    if (ACCUM) out[ra] = da + (p == p0 ? r0a : out[ra]); else out[ra] = da;
    if (rb < N) { if (ACCUM) out[rb] = db + (p == p0 ? r0b : out[rb]); else out[rb] = db; }
  };
  run_pairs_w4<DT, false, U, PFC>(map, epi, xs, K, npairs, p0, gridDim.x * kGemvWaves, pre);
}

// ---------------------------------------------------------------------------
// RMSNorm(f32 row) then f32 output over MXFP4 rows: the quantised lm_head, the 4-bit twin
// of gemv_norm_f32_kernel (SEL: + greedy selection, see HeadSel; the next input row comes
// from the 16-bit embedding table).  run_pairs_w4 delivers scaled sums, so the epilogue and
// tail are the 16-bit kernel's.
// ---------------------------------------------------------------------------
template <int DT, int U, int PFC, int NX, bool SEL>
__global__ __launch_bounds__(kGemvThreads) void gemv_norm_f32_w4_kernel(
    const float* __restrict__ resid, const uint16_t* __restrict__ norm_w, float eps,
    const uint8_t* __restrict__ w, const uint8_t* __restrict__ e8, int K, int N,
    float* __restrict__ out, HeadSel hs) {
  extern __shared__ float xs[];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int npairs = (N + 1) >> 1;
  const int p0 = blockIdx.x * kGemvWaves + wave;
  const size_t rowb = (size_t)K >> 1, rowe = (size_t)K >> 5;
  auto map = [&](int p) {
    const size_t ra = (size_t)(2 * p), rb = (size_t)min(2 * p + 1, N - 1);
    return RowsW4{w + ra * rowb, w + rb * rowb, e8 + ra * rowe, e8 + rb * rowe};
  };
  int hlen = 0;
  if constexpr (SEL) hlen = hs.penalty != 1.f ? *hs.hist_len : 0;
  RegsW4<PFC> pre;
  NormPreW4<DT, NX> xp;
  const RowsW4 r0 = map(p0 < npairs ? p0 : npairs - 1);
  if constexpr (NX > 0) xp.load(resid, norm_w, K);
  __builtin_amdgcn_sched_barrier(0);  // x loads strictly before the weights (in-order vmcnt)
  if (NX > 0 || (PFC > 0 && p0 < npairs)) prefetch_rows_w4<PFC>(r0, pre);  // NX: exact vmcnt
  __builtin_amdgcn_sched_barrier(0);
  if constexpr (NX > 0) xp.finish(eps, K, xs);
  else stage_rmsnorm_perm4<DT>(resid, norm_w, eps, K, xs);
  int win[4] = {-1, -1, -1, -1};
  if constexpr (SEL) head_sel_window(hs, hlen, lane, win);
  unsigned long long best = 0ull;
  auto epi = [&](int p, float da, float db) {
    const int ra = 2 * p, rb = 2 * p + 1;
    if constexpr (SEL) head_sel_pair(hs, win, ra, rb, N, da, db, best);
    if (lane != 0) return;
    out[ra] = da;
    if (rb < N) out[rb] = db;
  };
  run_pairs_w4<DT, true, U, PFC>(map, epi, xs, K, npairs, p0, gridDim.x * kGemvWaves, pre);
  if constexpr (SEL) head_sel_tail<DT>(hs, best, xs);
}

// Launch geometry of the MXFP4 launchers (their own table).  A row is K / 32 chunks:
// 8B's K = 4096 is 2 per lane, 70B's K = 8192 is 4, the down projections 7 and 14.  So the
// prefetch depths are PF in {0, 2, 4} chunks per row per lane (2 = the whole row of an 8B
// hidden-width projection, 4 = of a 70B one) and U in {1, 2, 4} for what follows it.
enum GemvW4Kind { kQkvW4 = 0, kSwigluW4 = 1, kX16W4 = 2, kHeadW4 = 3, kNumW4Kinds = 4 };
extern GemvTune g_tune_w4[kNumW4Kinds];  // defined in gemv_w4.hip (cake_gemv_w4_set_tuning)

}  // namespace cake

#define CAKE_W4_TUNE_U(PFCV, ...)                                                    \
  if (t.U == 1) { constexpr int U = 1; constexpr int PF = PFCV; __VA_ARGS__; }       \
  else if (t.U == 2) { constexpr int U = 2; constexpr int PF = PFCV; __VA_ARGS__; }  \
  else { constexpr int U = 4; constexpr int PF = PFCV; __VA_ARGS__; }
// the deepest prefetch <= t.PF that the row fills: PF 4 on a 128-chunk row runs as 2, and
// any depth as 0 when the row is shorter than 128 chunks
#define DISPATCH_W4_TUNE(t, K, ...)                                                  \
  do {                                                                               \
    const int nch_ = (K) / 32;                                                       \
    const int pfc_ = ((t).PF >= 4 && nch_ >= 256) ? 4 : (((t).PF >= 2 && nch_ >= 128) ? 2 : 0); \
    if (pfc_ == 4) { CAKE_W4_TUNE_U(4, __VA_ARGS__) }                                \
    else if (pfc_ == 2) { CAKE_W4_TUNE_U(2, __VA_ARGS__) }                           \
    else { CAKE_W4_TUNE_U(0, __VA_ARGS__) }                                          \
  } while (0)
