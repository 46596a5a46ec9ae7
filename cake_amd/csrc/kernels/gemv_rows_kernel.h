// MFMA GEMV for 1..16 activation rows: out[m, n] = sum_k x[m, k] w[n, k], the projection of a
// lock-step batched decode step.  The weights are streamed once for all rows (the per-row-pair
// VALU kernels of gemv_kernel.h would stream them once per row; the prefill GEMM tiles are 64
// or more rows tall).
//
// Shape of the work (v_mfma_f32_16x16x32, common.h cmfma):
//   * A operand = 16 weight rows x 32 k: lane l loads w[n0 + (l & 15)][k0 + 8 (l >> 4) .. + 8],
//     one non-temporal 16-byte load straight from global memory into the operand registers (no
//     LDS round trip: a weight byte is used by exactly one wave).
//   * B operand = 32 k x 16 activation rows: lane l loads x[l & 15][k0 + 8 (l >> 4) .. + 8] (L2
//     resident); lanes of rows >= M hold zeros and issue no load.  One x fragment serves the R
//     weight tiles (swiglu: R gate and R up tiles) a wave works on.
//   * D[4 (l >> 4) + e][l & 15] = element e of lane l: weight row down, activation row across, so
//     a lane ends with four consecutive output columns of one activation row.
//   * A workgroup is 8 waves on one group of R row tiles; wave v takes the 32-element k steps
//     v, v + 8, ...  (at each step the eight waves read 512 contiguous bytes of every row).  The
//     partial tiles meet in LDS and wave t sums tile t in wave order 0..7: no atomics, and the
//     sum order of out[m, n] depends on K alone -- not on M, not on the slot m sits in, not on
//     R, U or the grid -- which is what makes a batched decode bit-identical per sequence.
//   * Weight rows >= N are clamped to row N - 1 (loaded, never stored); output rows >= M and
//     columns >= N are never written.
#pragma once

#include "common.h"

namespace cake {

constexpr int kRowsWaves = 8, kRowsThreads = 64 * kRowsWaves;
constexpr int kRowsMinGroups = 512;  // R is halved while the grid would be below 2 blocks per CU

struct RowsTune { int tiles, unroll, max_blocks; };

struct RowsArgs {
  const uint16_t* x;  // [M, K], row stride ldx
  const uint16_t* w;  // [N, K] (swiglu: gate rows [0, N) and up rows [N, 2N)), row stride ldw
  void* out;          // store32: f32 [M, N]; swiglu: 16-bit [M, N]; row stride ldo
  float* resid;       // resid32: f32 [M, N] += , row stride ldr
  long long ldx, ldw, ldo, ldr;
  int M, N, K, ngroups;
};

template <int DT, int EPI, int R, int U>
__global__ __launch_bounds__(kRowsThreads) void gemv_rows_kernel(const RowsArgs a) {
  constexpr int NA = EPI == kEpiSwiglu ? 2 : 1;  // accumulators per row tile (gate, up)
  constexpr int NT = R * NA;
  __shared__ float4 part[kRowsWaves][NT][64];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int fr = lane & 15, fq = lane >> 4;
  const int KS = a.K >> 5;
  const bool xact = fr < a.M;
  const uint16_t* xp = a.x + (size_t)fr * a.ldx + 8 * fq;  // read only where xact
  for (int g = blockIdx.x; g < a.ngroups; g += gridDim.x) {
    const int n0 = g * (16 * R);
    const uint16_t* wp[NT];
#pragma unroll
    for (int t = 0; t < R; ++t) {
      const int row = min(n0 + 16 * t + fr, a.N - 1);
      wp[t * NA] = a.w + (size_t)row * a.ldw + 8 * fq;
      if constexpr (NA == 2) wp[t * NA + 1] = a.w + ((size_t)a.N + row) * a.ldw + 8 * fq;
    }
    cf32x4 acc[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[j] = cf32x4{0.f, 0.f, 0.f, 0.f};
    int s = wave;
    // U k steps per trip: every load of the trip is issued before its first MFMA
    for (; s + (U - 1) * kRowsWaves < KS; s += U * kRowsWaves) {
      uint4 wv[U][NT], xv[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const size_t k = (size_t)(s + u * kRowsWaves) << 5;
#pragma unroll
        for (int j = 0; j < NT; ++j) wv[u][j] = ld_nt16(reinterpret_cast<const uint4*>(wp[j] + k));
        xv[u] = make_uint4(0u, 0u, 0u, 0u);
        if (xact) xv[u] = *reinterpret_cast<const uint4*>(xp + k);
      }
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[j] = cmfma<DT>(wv[u][j], xv[u], acc[j]);
    }
    for (; s < KS; s += kRowsWaves) {
      const size_t k = (size_t)s << 5;
      uint4 wv[NT], xv = make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
      for (int j = 0; j < NT; ++j) wv[j] = ld_nt16(reinterpret_cast<const uint4*>(wp[j] + k));
      if (xact) xv = *reinterpret_cast<const uint4*>(xp + k);
#pragma unroll
      for (int j = 0; j < NT; ++j) acc[j] = cmfma<DT>(wv[j], xv, acc[j]);
    }
#pragma unroll
    for (int j = 0; j < NT; ++j)
      part[wave][j][lane] = make_float4(acc[j][0], acc[j][1], acc[j][2], acc[j][3]);
    __syncthreads();
    if (wave < R) {  // wave t finishes row tile t: partial sums in wave order
      float sum[NA][4];
#pragma unroll
      for (int j = 0; j < NA; ++j) {
        float4 v = part[0][wave * NA + j][lane];
#pragma unroll
        for (int w = 1; w < kRowsWaves; ++w) {
          const float4 p = part[w][wave * NA + j][lane];
          v.x += p.x; v.y += p.y; v.z += p.z; v.w += p.w;
        }
        sum[j][0] = v.x; sum[j][1] = v.y; sum[j][2] = v.z; sum[j][3] = v.w;
      }
      if (xact) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int n = n0 + 16 * wave + 4 * fq + e;
          if (n >= a.N) continue;
          if constexpr (EPI == kEpiStore32) {
            static_cast<float*>(a.out)[(size_t)fr * a.ldo + n] = sum[0][e];
          } else if constexpr (EPI == kEpiResid32) {
            a.resid[(size_t)fr * a.ldr + n] += sum[0][e];
          } else {
            static_cast<uint16_t*>(a.out)[(size_t)fr * a.ldo + n] =
                from_f32<DT>(silu(sum[0][e]) * sum[1][e]);
          }
        }
      }
    }
    __syncthreads();  // part is rewritten by the next group
  }
}

}  // namespace cake
