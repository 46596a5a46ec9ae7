// Decode GEMV kernels over FP8 (OCP e4m3fn) weight-only projections: the 8-bit twins of
// qkv_rope_kernel / swiglu_kernel / gemv_x16_kernel / gemv_norm_f32_kernel (gemv_kernel.h),
// shared by gemv_w8.hip, gemv_w8_mlp.hip, gemv_w8_x16.hip and gemv_w8_head.hip (one launcher
// per translation unit so the instantiations compile in parallel).
//
// Format: w8[N, K] one e4m3fn code per element, scale[N] f32 per output row,
// W[n, k] = scale[n] * fp8(w8[n, k])  (quant_fp8.hip writes it).  K % 16 == 0.
//
// Same structure as the 16-bit kernels: one wave per pair of rows, the x prologue loads
// issued before the wave's first weight rows, the first pair prefetched in registers,
// 16-byte non-temporal loads, wave_sum reductions, compile-time register indices.  A
// 16-byte chunk now carries 16 k values; the dot product accumulates the unscaled codes
// in f32 (two codes per v_cvt_pk_f32_fp8) and the row scale multiplies the wave sum once
// in the epilogue.  The scales of the wave's first pair are requested in the prologue,
// with the other epilogue operands.
#pragma once
#include "gemv_kernel.h"

namespace cake {

typedef float f32x2 __attribute__((ext_vector_type(2)));

// The f32 x row (RMSNorm output) is kept in LDS in a permuted order: a lane's chunk is 16
// floats = 64 bytes, and 64-byte lane strides are a 4-way bank conflict on ds_read_b128
// (16-lane groups over a 256-byte bank row).  Within every block of 64 chunks (1024
// floats) the j-th float4 of chunk l sits at float4 index j * 64 + l, so each of a lane's
// four reads is contiguous across the wave.  LDS holds K rounded up to 1024 floats.
__device__ __forceinline__ int x32_perm(int i) {  // i % 4 == 0: index of a float4's first float
  return (i & ~1023) | (((i >> 2) & 3) << 8) | (((i & 1023) >> 4) << 2);
}
static inline size_t x32_lds_bytes(int K) { return (size_t)((K + 1023) & ~1023) * sizeof(float); }

template <int DT>
__device__ __forceinline__ void stage_rmsnorm_perm(const float* __restrict__ x,
                                                   const uint16_t* __restrict__ w, float eps,
                                                   int K, float* xs) {
  __shared__ float red[16];
  float ss = 0.f;
  for (int i = threadIdx.x * 4; i < K; i += kGemvThreads * 4) {
    const float4 v = *reinterpret_cast<const float4*>(x + i);
    *reinterpret_cast<float4*>(xs + x32_perm(i)) = v;
    ss += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
  }
  ss = block_sum(ss, red);
  const float r = rsqrtf(ss / (float)K + eps);
  for (int i = threadIdx.x * 4; i < K; i += kGemvThreads * 4) {
    float4 v = *reinterpret_cast<float4*>(xs + x32_perm(i));
    const uint2 wv = *reinterpret_cast<const uint2*>(w + i);
    v.x *= r * to_f32<DT>((uint16_t)(wv.x & 0xffff));
    v.y *= r * to_f32<DT>((uint16_t)(wv.x >> 16));
    v.z *= r * to_f32<DT>((uint16_t)(wv.y & 0xffff));
    v.w *= r * to_f32<DT>((uint16_t)(wv.y >> 16));
    *reinterpret_cast<float4*>(xs + x32_perm(i)) = v;
  }
  __syncthreads();
}

// NormPre (gemv_kernel.h) with the permuted LDS image
template <int DT, int NX> struct NormPreW8 : NormPre<DT, NX> {
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
      if (i < K) *reinterpret_cast<float4*>(xs + x32_perm(i)) = v;
    }
    __syncthreads();
  }
};

// the 16 x values of a chunk
template <int DT, bool XF32>
__device__ __forceinline__ void load_x16(const void* xs, int chunk, float* o) {
  if constexpr (XF32) {
    const float4* p = reinterpret_cast<const float4*>(xs) + ((chunk >> 6) << 8) + (chunk & 63);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float4 a = p[j * 64];
      o[4 * j] = a.x; o[4 * j + 1] = a.y; o[4 * j + 2] = a.z; o[4 * j + 3] = a.w;
    }
  } else {
    const uint4* p = reinterpret_cast<const uint4*>(xs) + chunk * 2;
    unpack8<DT>(p[0], o);
    unpack8<DT>(p[1], o + 8);
  }
}

// two fp8 codes of a dword -> f32 (v_cvt_pk_f32_fp8; HI selects the upper 16 bits)
template <bool HI> __device__ __forceinline__ f32x2 fp8x2_to_f32(uint32_t w) {
  return __builtin_amdgcn_cvt_pk_f32_fp8((int)w, HI);
}

template <int DT, bool XF32>
__device__ __forceinline__ void fma_chunk_w8(const void* xs, int chunk, const uint4 va,
                                             const uint4 vb, f32x2& acc_a, f32x2& acc_b) {
  float xv[16];
  load_x16<DT, XF32>(xs, chunk, xv);
  const uint32_t wa[4] = {va.x, va.y, va.z, va.w};
  const uint32_t wb[4] = {vb.x, vb.y, vb.z, vb.w};
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    const f32x2 x01 = {xv[4 * d], xv[4 * d + 1]}, x23 = {xv[4 * d + 2], xv[4 * d + 3]};
    acc_a = __builtin_elementwise_fma(fp8x2_to_f32<false>(wa[d]), x01, acc_a);
    acc_b = __builtin_elementwise_fma(fp8x2_to_f32<false>(wb[d]), x01, acc_b);
    acc_a = __builtin_elementwise_fma(fp8x2_to_f32<true>(wa[d]), x23, acc_a);
    acc_b = __builtin_elementwise_fma(fp8x2_to_f32<true>(wb[d]), x23, acc_b);
  }
}

// accumulate chunks [c_start, nch) of rows wa, wb (c_start a multiple of 64)
template <int DT, bool XF32, int U>
__device__ __forceinline__ void dot_range_w8(const uint8_t* __restrict__ wa,
                                             const uint8_t* __restrict__ wb, const void* xs,
                                             int nch, int c_start, f32x2& acc_a, f32x2& acc_b) {
  const int lane = threadIdx.x & 63;
  const uint4* a4 = reinterpret_cast<const uint4*>(wa);
  const uint4* b4 = reinterpret_cast<const uint4*>(wb);
  const int full = c_start + ((nch - c_start) / (64 * U)) * (64 * U);
  for (int c0 = c_start; c0 < full; c0 += 64 * U) {
    uint4 va[U], vb[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      va[u] = ld_nt16(a4 + c0 + u * 64 + lane);
      vb[u] = ld_nt16(b4 + c0 + u * 64 + lane);
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
      fma_chunk_w8<DT, XF32>(xs, c0 + u * 64 + lane, va[u], vb[u], acc_a, acc_b);
  }
  for (int c = full + lane; c < nch; c += 64) fma_chunk_w8<DT, XF32>(xs, c, a4[c], b4[c], acc_a, acc_b);
}

// issue the first PFC chunks of (wa, wb)
template <int PFC>
__device__ __forceinline__ void prefetch_rows_w8(const uint8_t* wa, const uint8_t* wb, Regs<PFC>& r) {
  if constexpr (PFC > 0) {
    const int lane = threadIdx.x & 63;
    const uint4* a4 = reinterpret_cast<const uint4*>(wa);
    const uint4* b4 = reinterpret_cast<const uint4*>(wb);
#pragma unroll
    for (int c = 0; c < PFC; ++c) {
      r.a[c] = ld_nt16(a4 + c * 64 + lane);
      r.b[c] = ld_nt16(b4 + c * 64 + lane);
    }
  }
}

// run_pairs (gemv_kernel.h) over byte rows; epi gets the UNSCALED dot products
template <int DT, bool XF32, int U, int PFC, class Map, class Epi>
__device__ __forceinline__ void run_pairs_w8(const Map& map, const Epi& epi, const void* xs, int K,
                                             int npairs, int p0, int stride, const Regs<PFC>& pre) {
  const int nch = K >> 4;
  int p = p0;
  if constexpr (PFC > 0) {
    // unconditional, as in run_pairs: an idle wave works on a clamped pair and drops it
    const uint8_t *wa, *wb;
    map(p < npairs ? p : npairs - 1, wa, wb);
    const int lane = threadIdx.x & 63;
    f32x2 aa = {0.f, 0.f}, ab = {0.f, 0.f};
#pragma unroll
    for (int c = 0; c < PFC; ++c) fma_chunk_w8<DT, XF32>(xs, c * 64 + lane, pre.a[c], pre.b[c], aa, ab);
    dot_range_w8<DT, XF32, U>(wa, wb, xs, nch, PFC * 64, aa, ab);
    const float sa = wave_sum(aa.x + aa.y), sb = wave_sum(ab.x + ab.y);
    if (p < npairs) epi(p, sa, sb);
    p += stride;
  }
  for (; p < npairs; p += stride) {
    const uint8_t *wa, *wb;
    map(p, wa, wb);
    f32x2 aa = {0.f, 0.f}, ab = {0.f, 0.f};
    dot_range_w8<DT, XF32, U>(wa, wb, xs, nch, 0, aa, ab);
    epi(p, wave_sum(aa.x + aa.y), wave_sum(ab.x + ab.y));
  }
}

// ---------------------------------------------------------------------------
// QKV + RoPE + KV-cache write
// ---------------------------------------------------------------------------
struct QkvW8Args {
  const float* resid;      // [K] f32
  const uint16_t* norm_w;  // [K]
  float eps;
  const uint8_t* wq;  // [nh*hd, K] e4m3fn
  const uint8_t* wk;  // [nkv*hd, K]
  const uint8_t* wv;  // [nkv*hd, K]
  const float* sq;    // [nh*hd] row scales
  const float* sk;    // [nkv*hd]
  const float* sv;    // [nkv*hd]
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
__global__ __launch_bounds__(kGemvThreads) void qkv_rope_w8_kernel(QkvW8Args a) {
  extern __shared__ float xs[];
  const int half = a.hd >> 1;
  const int npairs = (a.nh + 2 * a.nkv) * half;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int p0 = blockIdx.x * kGemvWaves + wave;
  // bases selected by address arithmetic, not a pointer select (see qkv_rope_kernel)
  const uint8_t* wq = a.wq;
  const float* sq = a.sq;
  const ptrdiff_t dk = a.wk - a.wq, dv = a.wv - a.wq;
  const ptrdiff_t dsk = a.sk - a.sq, dsv = a.sv - a.sq;
  const int nh = a.nh, nqk = a.nh + a.nkv, hd = a.hd, K = a.K;
  // kind 0 = q, 1 = k, 2 = v; ra = the pair's first row inside its matrix
  auto where = [=](int p, int& kind, int& head, size_t& ra) {
    const int slot = p / half;
    const bool isq = slot < nh, isk = !isq && slot < nqk;
    kind = isq ? 0 : (isk ? 1 : 2);
    head = slot - (isq ? 0 : (isk ? nh : nqk));
    ra = (size_t)head * hd + (p - slot * half);
  };
  auto map = [=](int p, const uint8_t*& wa, const uint8_t*& wb) {
    int kind, head;
    size_t ra;
    where(p, kind, head, ra);
    const uint8_t* base = wq + (kind == 0 ? 0 : (kind == 1 ? dk : dv));
    wa = base + ra * K;
    wb = base + (ra + half) * K;
  };
  auto scales = [=](int p, float& sa, float& sb) {
    int kind, head;
    size_t ra;
    where(p, kind, head, ra);
    const float* base = sq + (kind == 0 ? 0 : (kind == 1 ? dsk : dsv));
    sa = base[ra];
    sb = base[ra + half];
  };
  Regs<PFC> pre;
  NormPreW8<DT, NX> xp;
  const int pc = p0 < npairs ? p0 : npairs - 1;
  const uint8_t *wa0, *wb0;  // rows first: their address math may load (kernarg select)
  map(pc, wa0, wb0);
  if constexpr (NX > 0) xp.load(a.resid, a.norm_w, a.K);
  __builtin_amdgcn_sched_barrier(0);  // x loads strictly before the weights (in-order vmcnt)
  if (NX > 0 || (PFC > 0 && p0 < npairs)) prefetch_rows_w8<PFC>(wa0, wb0, pre);  // NX: exact vmcnt
  // the first pair's epilogue operands, requested now: RoPE frequency and row scales
  const float f0 = a.inv_freq[pc - (pc / half) * half];
  float s0a, s0b;
  scales(pc, s0a, s0b);
  __builtin_amdgcn_sched_barrier(0);
  if constexpr (NX > 0) xp.finish(a.eps, a.K, xs);
  else stage_rmsnorm_perm<DT>(a.resid, a.norm_w, a.eps, a.K, xs);
  const int pos = *a.pos;
  auto epi = [&](int p, float da, float db) {
    if (lane != 0) return;
    int kind, head;
    size_t ra;
    where(p, kind, head, ra);
    const int i = p - (p / half) * half;
    float sa = s0a, sb = s0b;
    if (p != p0) scales(p, sa, sb);
    da *= sa;
    db *= sb;
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
  run_pairs_w8<DT, true, U, PFC>(map, epi, xs, a.K, npairs, p0, gridDim.x * kGemvWaves, pre);
}

// ---------------------------------------------------------------------------
// RMSNorm + gate/up + SiLU*mul
// ---------------------------------------------------------------------------
template <int DT, int U, int PFC, int NX>
__global__ __launch_bounds__(kGemvThreads) void swiglu_w8_kernel(
    const float* __restrict__ resid, const uint16_t* __restrict__ norm_w, float eps,
    const uint8_t* __restrict__ wg, const uint8_t* __restrict__ wu,
    const float* __restrict__ sg, const float* __restrict__ su, int K, int I,
    uint16_t* __restrict__ act) {
  extern __shared__ float xs[];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int j0 = blockIdx.x * kGemvWaves + wave;
  auto map = [&](int j, const uint8_t*& wa, const uint8_t*& wb) {
    wa = wg + (size_t)j * K;
    wb = wu + (size_t)j * K;
  };
  Regs<PFC> pre;
  NormPreW8<DT, NX> xp;
  const int jp = j0 < I ? j0 : I - 1;
  const uint8_t *wa0 = wg + (size_t)jp * K, *wb0 = wu + (size_t)jp * K;
  if constexpr (NX > 0) xp.load(resid, norm_w, K);
  __builtin_amdgcn_sched_barrier(0);  // x loads strictly before the weights (in-order vmcnt)
  // NX: unconditional (an idle wave re-reads the last row), so the vmcnt is exact
  if (NX > 0 || (PFC > 0 && j0 < I)) prefetch_rows_w8<PFC>(wa0, wb0, pre);
  const float s0g = sg[jp], s0u = su[jp];  // the first pair's scales, requested now
  __builtin_amdgcn_sched_barrier(0);
  if constexpr (NX > 0) xp.finish(eps, K, xs);
  else stage_rmsnorm_perm<DT>(resid, norm_w, eps, K, xs);
  auto epi = [&](int j, float g, float u) {
    if (lane != 0) return;
    const float a = j == j0 ? s0g : sg[j], b = j == j0 ? s0u : su[j];
    act[j] = from_f32<DT>(silu(g * a) * (u * b));
  };
  run_pairs_w8<DT, true, U, PFC>(map, epi, xs, K, I, j0, gridDim.x * kGemvWaves, pre);
}

// ---------------------------------------------------------------------------
// out (+)= W x   with 16-bit x: o_proj / down_proj
// ---------------------------------------------------------------------------
template <int DT, int U, int PFC, int NX, bool ACCUM>
__global__ __launch_bounds__(kGemvThreads) void gemv_x16_w8_kernel(
    const uint16_t* __restrict__ x, const uint8_t* __restrict__ w,
    const float* __restrict__ scale, int K, int N, float* __restrict__ out) {
  extern __shared__ float smem[];
  uint16_t* xs = reinterpret_cast<uint16_t*>(smem);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int npairs = (N + 1) >> 1;
  const int p0 = blockIdx.x * kGemvWaves + wave;
  auto map = [&](int p, const uint8_t*& wa, const uint8_t*& wb) {
    wa = w + (size_t)(2 * p) * K;
    wb = w + (size_t)min(2 * p + 1, N - 1) * K;
  };
  Regs<PFC> pre;
  Plain16Pre<NX> xp;
  const int pc = p0 < npairs ? p0 : npairs - 1;
  const uint8_t *wa0, *wb0;
  map(pc, wa0, wb0);
  if constexpr (NX > 0) xp.load(x, K);
  __builtin_amdgcn_sched_barrier(0);  // x loads strictly before the weights (in-order vmcnt)
  if (NX > 0 || (PFC > 0 && p0 < npairs)) prefetch_rows_w8<PFC>(wa0, wb0, pre);  // NX: exact vmcnt
  // the first pair's epilogue operands, requested now: row scales and (ACCUM) the
  // residual words (no other wave of this launch writes them)
  const float s0a = scale[2 * pc], s0b = scale[min(2 * pc + 1, N - 1)];
  float r0a = 0.f, r0b = 0.f;
  if constexpr (ACCUM) {
    r0a = out[2 * pc];
    r0b = out[min(2 * pc + 1, N - 1)];
  }
  __builtin_amdgcn_sched_barrier(0);
  if constexpr (NX > 0) xp.finish(K, xs);
  else stage_plain16(x, K, xs);
  auto epi = [&](int p, float da, float db) {
    if (lane != 0) return;
    const int ra = 2 * p, rb = 2 * p + 1;
    da *= p == p0 ? s0a : scale[ra];
    if (ACCUM) out[ra] = da + (p == p0 ? r0a : out[ra]); else out[ra] = da;
    if (rb < N) {
      db *= p == p0 ? s0b : scale[rb];
      if (ACCUM) out[rb] = db + (p == p0 ? r0b : out[rb]); else out[rb] = db;
    }
  };
  run_pairs_w8<DT, false, U, PFC>(map, epi, xs, K, npairs, p0, gridDim.x * kGemvWaves, pre);
}

// ---------------------------------------------------------------------------
// RMSNorm(f32 row) then f32 output over fp8 rows: the quantised lm_head, the 8-bit twin of
// gemv_norm_f32_kernel (SEL: + greedy selection, see HeadSel; the next input row comes
// from the 16-bit embedding table)
// ---------------------------------------------------------------------------
template <int DT, int U, int PFC, int NX, bool SEL>
__global__ __launch_bounds__(kGemvThreads) void gemv_norm_f32_w8_kernel(
    const float* __restrict__ resid, const uint16_t* __restrict__ norm_w, float eps,
    const uint8_t* __restrict__ w, const float* __restrict__ scale, int K, int N,
    float* __restrict__ out, HeadSel hs) {
  extern __shared__ float xs[];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int npairs = (N + 1) >> 1;
  const int p0 = blockIdx.x * kGemvWaves + wave;
  auto map = [&](int p, const uint8_t*& wa, const uint8_t*& wb) {
    wa = w + (size_t)(2 * p) * K;
    wb = w + (size_t)min(2 * p + 1, N - 1) * K;
  };
  // SEL: the history length ahead of the x prologue, the window after it (as the 16-bit
  // kernel)
  int hlen = 0;
  if constexpr (SEL) hlen = hs.penalty != 1.f ? *hs.hist_len : 0;
  Regs<PFC> pre;
  NormPreW8<DT, NX> xp;
  const int pc = p0 < npairs ? p0 : npairs - 1;
  const uint8_t *wa0, *wb0;
  map(pc, wa0, wb0);
  if constexpr (NX > 0) xp.load(resid, norm_w, K);
  __builtin_amdgcn_sched_barrier(0);  // x loads strictly before the weights (in-order vmcnt)
  if (NX > 0 || (PFC > 0 && p0 < npairs)) prefetch_rows_w8<PFC>(wa0, wb0, pre);  // NX: exact vmcnt
  // the first pair's row scales, requested now (one address per wave: every lane holds
  // the value, which the SEL ballot and key need wave-wide)
  const float s0a = scale[2 * pc], s0b = scale[min(2 * pc + 1, N - 1)];
  __builtin_amdgcn_sched_barrier(0);
  if constexpr (NX > 0) xp.finish(eps, K, xs);
  else stage_rmsnorm_perm<DT>(resid, norm_w, eps, K, xs);
  int win[4] = {-1, -1, -1, -1};
  if constexpr (SEL) head_sel_window(hs, hlen, lane, win);
  unsigned long long best = 0ull;
  auto epi = [&](int p, float da, float db) {
    const int ra = 2 * p, rb = 2 * p + 1;
    // the row scales first: everything below sees the logits
    da *= p == p0 ? s0a : scale[ra];
    db *= p == p0 ? s0b : scale[min(rb, N - 1)];
    if constexpr (SEL) head_sel_pair(hs, win, ra, rb, N, da, db, best);
    if (lane != 0) return;
    out[ra] = da;
    if (rb < N) out[rb] = db;
  };
  run_pairs_w8<DT, true, U, PFC>(map, epi, xs, K, npairs, p0, gridDim.x * kGemvWaves, pre);
  if constexpr (SEL) head_sel_tail<DT>(hs, best, xs);
}

// Launch geometry of the fp8 launchers (their own table: a row is half the bytes of
// its 16-bit twin — 8B's K = 4096 is 4 chunks per lane — so the 16-bit tuning does not
// carry over).  U in {1, 2, 4}, PF in {0, 2, 4} chunks per row per lane.
enum GemvW8Kind { kQkvW8 = 0, kSwigluW8 = 1, kX16W8 = 2, kHeadW8 = 3, kNumW8Kinds = 4 };
extern GemvTune g_tune_w8[kNumW8Kinds];  // defined in gemv_w8.hip (cake_gemv_w8_set_tuning)

}  // namespace cake

#define CAKE_W8_TUNE_U(PFCV, ...)                                                    \
  if (t.U == 1) { constexpr int U = 1; constexpr int PF = PFCV; __VA_ARGS__; }       \
  else if (t.U == 2) { constexpr int U = 2; constexpr int PF = PFCV; __VA_ARGS__; }  \
  else { constexpr int U = 4; constexpr int PF = PFCV; __VA_ARGS__; }
// PFC falls back to 0 when a row is shorter than PFC*64 chunks
#define DISPATCH_W8_TUNE(t, K, ...)                                                  \
  do {                                                                               \
    const int pfc_ = ((K) / 16 >= 64 * (t).PF) ? (t).PF : 0;                         \
    if (pfc_ == 4) { CAKE_W8_TUNE_U(4, __VA_ARGS__) }                                \
    else if (pfc_ == 2) { CAKE_W8_TUNE_U(2, __VA_ARGS__) }                           \
    else { CAKE_W8_TUNE_U(0, __VA_ARGS__) }                                          \
  } while (0)
