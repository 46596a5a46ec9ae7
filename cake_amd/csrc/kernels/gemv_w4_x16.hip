// MXFP4 weight-only decode entry point: the 16-bit-input GEMV (o_proj / down_proj,
// optional residual accumulate), cake_gemv_x16 (gemv_mlp.hip) with packed 4-bit weights
// and their block-scale bytes.
//
// This one kind of this one format is NOT gemv_x16_kernel<W4, ...> of the shared family
// (gemv_kernel.h): instantiated over W4, that kernel ran 70B's down_proj 1 % slower than
// the kernel below (26.4 -> 26.6 us per launch, +0.26 % per token against a run-to-run
// spread of 0.13 %; profiles/gemv_unify_ab.jsonl), for a reason that was not found (the
// streams differ by three instructions and two VGPRs; restoring __restrict__ on the shared
// kernel's pointers did not change them).  So the kernel and its pair loop stay as they
// were before the family was unified; only the x staging, the LDS layout and the chunk FMA
// come from the W4 policy.  Fold it into the family when that difference is understood.
#include "gemv_w4_kernel.h"

namespace cake {

// the code and scale rows of a pair
struct RowsW4 {
  const uint8_t *wa, *wb;  // [K/2] codes
  const uint8_t *ea, *eb;  // [K/32] scale bytes
};

// prefetch registers: PFC chunks per row per lane and their scale bytes
template <int N> struct RegsW4 { uint4 a[N], b[N]; uint32_t ea[N], eb[N]; };
template <> struct RegsW4<0> { uint4 a[1], b[1]; uint32_t ea[1], eb[1]; };

// one chunk of both rows: 32 k values, ea / eb the chunk's scale bytes
template <int DT>
__device__ __forceinline__ void fma_chunk_w4(const void* xs, int chunk, const uint4 va,
                                             const uint4 vb, uint32_t ea, uint32_t eb,
                                             f32x2_t& acc_a, f32x2_t& acc_b) {
  W4::fma<DT, false>(xs, chunk, W4::Chunk{va, vb, ea, eb}, acc_a, acc_b);
}

// accumulate chunks [c_start, nch) of the pair (c_start a multiple of 64)
template <int DT, int U>
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
      fma_chunk_w4<DT>(xs, c0 + u * 64 + lane, va[u], vb[u], ea[u], eb[u], acc_a, acc_b);
  }
  // the tail: lanes past nch have no chunk (K / 32 < 64: most of the wave)
  for (int c = full + lane; c < nch; c += 64)
    fma_chunk_w4<DT>(xs, c, a4[c], b4[c], r.ea[c], r.eb[c], acc_a, acc_b);
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

// run_pairs (gemv_kernel.h) over these rows
template <int DT, int U, int PFC, class Map, class Epi>
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
      fma_chunk_w4<DT>(xs, c * 64 + lane, pre.a[c], pre.b[c], pre.ea[c], pre.eb[c], aa, ab);
    dot_range_w4<DT, U>(r, xs, nch, PFC * 64, aa, ab);
    const float sa = wave_sum(aa.x + aa.y), sb = wave_sum(ab.x + ab.y);
    if (p < npairs) epi(p, sa, sb);
    p += stride;
  }
  for (; p < npairs; p += stride) {
    const RowsW4 r = map(p);
    f32x2_t aa = {0.f, 0.f}, ab = {0.f, 0.f};
    dot_range_w4<DT, U>(r, xs, nch, 0, aa, ab);
    epi(p, wave_sum(aa.x + aa.y), wave_sum(ab.x + ab.y));
  }
}

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
  Plain16Pre<W4, NX> xp;
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
  else stage_plain16<W4>(x, K, xs);
  auto epi = [&](int p, float da, float db) {
    if (lane != 0) return;
    const int ra = 2 * p, rb = 2 * p + 1;
    if (ACCUM) out[ra] = da + (p == p0 ? r0a : out[ra]); else out[ra] = da;
    if (rb < N) { if (ACCUM) out[rb] = db + (p == p0 ? r0b : out[rb]); else out[rb] = db; }
  };
  run_pairs_w4<DT, U, PFC>(map, epi, xs, K, npairs, p0, gridDim.x * kGemvWaves, pre);
}

}  // namespace cake

CAKE_API int cake_gemv_x16_w4(int dt, const void* x, const void* w, const void* e8, int K,
                              int N, float* out, int accumulate, hipStream_t st) {
  if (bad_shape<W4>(K, N)) return (int)hipErrorInvalidValue;
  const size_t lds = x16_lds_bytes<W4>(K);
  const GemvTune t = g_tune[W4::kFmt][kX16];
  const int g = grid_for((N + 1) / 2, t.MB);
  if (accumulate) {
    DISPATCH_DT(dt, DISPATCH_TUNE(W4, t, K, CAKE_NX_X16(K, hipLaunchKernelGGL((gemv_x16_w4_kernel<DT, U, PF, NX, true>),
                                                           dim3(g), dim3(kGemvThreads), lds, st,
                                                           (const uint16_t*)x, (const uint8_t*)w,
                                                           (const uint8_t*)e8, K, N, out))));
  } else {
    DISPATCH_DT(dt, DISPATCH_TUNE(W4, t, K, CAKE_NX_X16(K, hipLaunchKernelGGL((gemv_x16_w4_kernel<DT, U, PF, NX, false>),
                                                           dim3(g), dim3(kGemvThreads), lds, st,
                                                           (const uint16_t*)x, (const uint8_t*)w,
                                                           (const uint8_t*)e8, K, N, out))));
  }
  return (int)hipGetLastError();
}
