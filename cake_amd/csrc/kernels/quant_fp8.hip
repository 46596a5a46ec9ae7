// FP8 (OCP e4m3fn) weight-only storage of the decode projections: quantise on load,
// dequantise for prefill.
//
// Format: w8[N, K] one code per element, scale[N] f32 per row,
//   scale[n] = amax_n / 448 (IEEE f32 division; 1 when the row is all zero),
//   code     = rne_e4m3(clamp(float(w) / scale[n], -448, 448)),
//   W[n, k] ~= scale[n] * fp8(w8[n, k]).
// gfx950 converts OCP e4m3 natively (v_cvt_pk_fp8_f32 / v_cvt_pk_f32_fp8); the explicit
// clamp keeps the NaN code out whatever the conversion's overflow mode.
#include "common.h"

namespace cake {

constexpr int kQuantThreads = 256;
constexpr float kE4M3Max = 448.f;

__device__ __forceinline__ float block_max(float v, float* red) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  v = wave_max(v);
  if (lane == 0) red[wave] = v;
  __syncthreads();
  float t = red[0];
#pragma unroll
  for (int i = 1; i < kQuantThreads / 64; ++i) t = fmaxf(t, red[i]);
  return t;
}

template <int DT> __device__ __forceinline__ float amax8(const uint4 v, float m) {
  float f[8];
  unpack8<DT>(v, f);
#pragma unroll
  for (int e = 0; e < 8; ++e) m = fmaxf(m, fabsf(f[e]));
  return m;
}

// 8 16-bit weights -> 8 codes
template <int DT> __device__ __forceinline__ uint2 quant8(const uint4 v, float scale) {
  float f[8];
  unpack8<DT>(v, f);
#pragma unroll
  for (int e = 0; e < 8; ++e) f[e] = fminf(fmaxf(f[e] / scale, -kE4M3Max), kE4M3Max);
  int lo = 0, hi = 0;
  lo = __builtin_amdgcn_cvt_pk_fp8_f32(f[0], f[1], lo, false);
  lo = __builtin_amdgcn_cvt_pk_fp8_f32(f[2], f[3], lo, true);
  hi = __builtin_amdgcn_cvt_pk_fp8_f32(f[4], f[5], hi, false);
  hi = __builtin_amdgcn_cvt_pk_fp8_f32(f[6], f[7], hi, true);
  return make_uint2((uint32_t)lo, (uint32_t)hi);
}

// One workgroup per row, the row held in registers between the amax and the convert
// (NP passes of 256 x 8 elements: K <= 2048 NP).  NP = 0: any K, the row read twice.
template <int DT, int NP>
__global__ __launch_bounds__(kQuantThreads) void quant_rows_fp8_kernel(
    const uint16_t* __restrict__ w16, int K, uint8_t* __restrict__ w8,
    float* __restrict__ scale) {
  __shared__ float red[kQuantThreads / 64];
  const size_t row = blockIdx.x;
  const uint16_t* src = w16 + row * K;
  uint8_t* dst = w8 + row * K;
  float m = 0.f;
  if constexpr (NP > 0) {
    uint4 r[NP];
#pragma unroll
    for (int j = 0; j < NP; ++j) {
      const int i = (j * kQuantThreads + threadIdx.x) * 8;
      r[j] = i < K ? *reinterpret_cast<const uint4*>(src + i) : make_uint4(0u, 0u, 0u, 0u);
      m = amax8<DT>(r[j], m);
    }
    m = block_max(m, red);
    const float s = m == 0.f ? 1.f : m / kE4M3Max;
    if (threadIdx.x == 0) scale[row] = s;
#pragma unroll
    for (int j = 0; j < NP; ++j) {
      const int i = (j * kQuantThreads + threadIdx.x) * 8;
      if (i < K) *reinterpret_cast<uint2*>(dst + i) = quant8<DT>(r[j], s);
    }
  } else {
    for (int i = threadIdx.x * 8; i < K; i += kQuantThreads * 8)
      m = amax8<DT>(*reinterpret_cast<const uint4*>(src + i), m);
    m = block_max(m, red);
    const float s = m == 0.f ? 1.f : m / kE4M3Max;
    if (threadIdx.x == 0) scale[row] = s;
    for (int i = threadIdx.x * 8; i < K; i += kQuantThreads * 8)
      *reinterpret_cast<uint2*>(dst + i) = quant8<DT>(*reinterpret_cast<const uint4*>(src + i), s);
  }
}

// out16 = to_dt(scale[n] * fp8(w8)): one 16-byte load of codes, two 16-byte stores
template <int DT>
__global__ __launch_bounds__(256) void dequant_rows_fp8_kernel(
    const uint8_t* __restrict__ w8, const float* __restrict__ scale, size_t nchunks, int cpr,
    uint16_t* __restrict__ out) {
  for (size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x; c < nchunks;
       c += (size_t)gridDim.x * blockDim.x) {
    const uint4 v = reinterpret_cast<const uint4*>(w8)[c];
    const float s = scale[c / (size_t)cpr];
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    uint32_t o[8];
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      const auto lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[d], false);
      const auto hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[d], true);
      o[2 * d] = (uint32_t)from_f32<DT>(lo[0] * s) | ((uint32_t)from_f32<DT>(lo[1] * s) << 16);
      o[2 * d + 1] = (uint32_t)from_f32<DT>(hi[0] * s) | ((uint32_t)from_f32<DT>(hi[1] * s) << 16);
    }
    uint4* dst = reinterpret_cast<uint4*>(out) + 2 * c;
    dst[0] = make_uint4(o[0], o[1], o[2], o[3]);
    dst[1] = make_uint4(o[4], o[5], o[6], o[7]);
  }
}

}  // namespace cake

using namespace cake;

#define QUANT_DT(dt, ...)                                                \
  do {                                                                   \
    if ((dt) == kBF16) { constexpr int DT = kBF16; __VA_ARGS__; }        \
    else if ((dt) == kF16) { constexpr int DT = kF16; __VA_ARGS__; }     \
    else return (int)hipErrorInvalidValue;                               \
  } while (0)

CAKE_API int cake_quant_rows_fp8(int dt, const void* w16, int N, int K, void* w8, float* scale,
                                 hipStream_t st) {
  if (K < 16 || K % 16 || N < 1) return (int)hipErrorInvalidValue;
  const uint16_t* src = (const uint16_t*)w16;
  uint8_t* dst = (uint8_t*)w8;
#define QUANT_LAUNCH(NPV)                                                                  \
  hipLaunchKernelGGL((quant_rows_fp8_kernel<DT, NPV>), dim3(N), dim3(kQuantThreads), 0, st, \
                     src, K, dst, scale)
  QUANT_DT(dt, {
    if (K <= 2048) QUANT_LAUNCH(1);
    else if (K <= 4096) QUANT_LAUNCH(2);
    else if (K <= 8192) QUANT_LAUNCH(4);
    else if (K <= 16384) QUANT_LAUNCH(8);
    else if (K <= 32768) QUANT_LAUNCH(16);
    else QUANT_LAUNCH(0);
  });
#undef QUANT_LAUNCH
  return (int)hipGetLastError();
}

CAKE_API int cake_dequant_rows_fp8(int dt, const void* w8, const float* scale, int N, int K,
                                   void* out16, hipStream_t st) {
  if (K < 16 || K % 16 || N < 1) return (int)hipErrorInvalidValue;
  const int cpr = K / 16;
  const size_t nchunks = (size_t)N * cpr;
  const size_t want = (nchunks + 255) / 256;
  const int grid = (int)(want < 8192 ? want : 8192);
  QUANT_DT(dt, hipLaunchKernelGGL((dequant_rows_fp8_kernel<DT>), dim3(grid), dim3(256), 0, st,
                                  (const uint8_t*)w8, scale, nchunks, cpr, (uint16_t*)out16));
  return (int)hipGetLastError();
}
