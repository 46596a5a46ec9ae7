// OCP MXFP4 weight-only storage of the decode projections: quantise on load, dequantise
// for prefill.
//
// Format (fixed by ops/reference.py quant_rows_mxfp4): a row of W[N, K], K % 32 == 0, is
// K/32 blocks of 32 consecutive k.
//   e8[n, b]  = e + 127,  e = clamp(floor(log2(amax_block)) - 2, -126, 127)  (127 when the
//               block is all zero): an e8m0 power-of-two scale, never 0xFF,
//   code      = s e e m (e2m1): |w / 2^e| saturated to 6, rounded to the nearest of
//               {0, .5, 1, 1.5, 2, 3, 4, 6}, ties to the even code; s = the sign bit of w,
//   w4[n, i]  = code(k = 2i) | code(k = 2i + 1) << 4,
//   W[n, k]  ~= 2^(e8[n, k / 32] - 127) * e2m1(code).
// The quantiser rounds with compares in plain C++ (tie rule and saturation are then the
// oracle's by construction); the dequantiser uses gfx950's v_cvt_scalef32_pk_f32_fp4,
// which applies the block scale inside the convert (kernel tests: bit-equal to the oracle).
#include "mxfp4.h"

namespace cake {

constexpr int kQuantThreads = 256;

// max over the four lanes of a quad (quad_perm xor 1, xor 2): one 32-element block
__device__ __forceinline__ float quad_max(float v) {
  v = fmaxf(v, dpp_f<kDppXor1>(v));
  return fmaxf(v, dpp_f<kDppXor2>(v));
}
// lane K's value of the quad, in every lane of it (quad_perm [K, K, K, K])
template <int K> __device__ __forceinline__ uint32_t quad_bcast(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, K * 0x55, 0xF, 0xF, false);
}

// e2m1 code of w under the block exponent whose inverse is inv = 2^-e
__device__ __forceinline__ uint32_t e2m1_code(float w, float inv) {
  const float a = fabsf(w) * inv;  // exact: a power of two, |w| < 2^(e + 3)
  const uint32_t mag = (a > 0.25f) + (a >= 0.75f) + (a > 1.25f) + (a >= 1.75f) + (a > 2.5f) +
                       (a >= 3.5f) + (a > 5.f);
  return mag | ((__float_as_uint(w) >> 31) << 3);
}

// A lane holds 8 consecutive weights (one 16-byte load), a quad one block: amax over the
// quad, 8 codes = 4 bytes per lane, the quad's 16 bytes stored by its first lane.  K % 32
// == 0, so a block never straddles rows and the matrix is one run of N K / 32 blocks.
template <int DT>
__global__ __launch_bounds__(kQuantThreads) void quant_rows_mxfp4_kernel(
    const uint16_t* __restrict__ w16, size_t nchunks, uint8_t* __restrict__ w4,
    uint8_t* __restrict__ e8) {
  // nchunks % 4 == 0 and the stride is a multiple of 4: a quad is in or out as one
  for (size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x; c < nchunks;
       c += (size_t)gridDim.x * blockDim.x) {
    float f[8];
    unpack8<DT>(reinterpret_cast<const uint4*>(w16)[c], f);
    float m = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) m = fmaxf(m, fabsf(f[i]));
    m = quad_max(m);
    // floor(log2 m) = the exponent field - 127 (a subnormal amax clamps to -126 either way)
    int e = (int)(__float_as_uint(m) >> 23) - 127 - 2;
    e = e < -126 ? -126 : e;  // the field is at most 254 + 1: e <= 126
    if (m == 0.f) e = 0;
    const float inv = __uint_as_float((uint32_t)(127 - e) << 23);
    uint32_t word = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) word |= e2m1_code(f[i], inv) << (4 * i);
    const uint4 out = make_uint4(quad_bcast<0>(word), quad_bcast<1>(word), quad_bcast<2>(word),
                                 quad_bcast<3>(word));
    if ((threadIdx.x & 3) == 0) {
      reinterpret_cast<uint4*>(w4)[c >> 2] = out;
      e8[c >> 2] = (uint8_t)(e + 127);
    }
  }
}

// out16 = to_dt(2^(e8 - 127) * e2m1(code)): a lane takes one block (16 bytes of codes,
// one scale byte) and stores its 32 values as four 16-byte words
template <int DT>
__global__ __launch_bounds__(256) void dequant_rows_mxfp4_kernel(
    const uint8_t* __restrict__ w4, const uint8_t* __restrict__ e8, size_t nblocks,
    uint16_t* __restrict__ out) {
  for (size_t b = (size_t)blockIdx.x * blockDim.x + threadIdx.x; b < nblocks;
       b += (size_t)gridDim.x * blockDim.x) {
    const uint4 v = reinterpret_cast<const uint4*>(w4)[b];
    const float s = e8m0_to_f32(e8[b]);
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    uint4* dst = reinterpret_cast<uint4*>(out) + 4 * b;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      const f32x2_t p0 = fp4x2_to_f32<0>(w[d], s), p1 = fp4x2_to_f32<1>(w[d], s);
      const f32x2_t p2 = fp4x2_to_f32<2>(w[d], s), p3 = fp4x2_to_f32<3>(w[d], s);
      dst[d] = make_uint4(
          (uint32_t)from_f32<DT>(p0[0]) | ((uint32_t)from_f32<DT>(p0[1]) << 16),
          (uint32_t)from_f32<DT>(p1[0]) | ((uint32_t)from_f32<DT>(p1[1]) << 16),
          (uint32_t)from_f32<DT>(p2[0]) | ((uint32_t)from_f32<DT>(p2[1]) << 16),
          (uint32_t)from_f32<DT>(p3[0]) | ((uint32_t)from_f32<DT>(p3[1]) << 16));
    }
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

static inline int quant_grid(size_t n, int threads) {
  const size_t want = (n + threads - 1) / threads;
  return (int)(want < 8192 ? want : 8192);
}

CAKE_API int cake_quant_rows_mxfp4(int dt, const void* w16, int N, int K, void* w4, void* e8,
                                   hipStream_t st) {
  if (K < 32 || K % 32 || N < 1) return (int)hipErrorInvalidValue;
  const size_t nchunks = (size_t)N * (K / 8);
  QUANT_DT(dt, hipLaunchKernelGGL((quant_rows_mxfp4_kernel<DT>),
                                  dim3(quant_grid(nchunks, kQuantThreads)), dim3(kQuantThreads), 0,
                                  st, (const uint16_t*)w16, nchunks, (uint8_t*)w4, (uint8_t*)e8));
  return (int)hipGetLastError();
}

CAKE_API int cake_dequant_rows_mxfp4(int dt, const void* w4, const void* e8, int N, int K,
                                     void* out16, hipStream_t st) {
  if (K < 32 || K % 32 || N < 1) return (int)hipErrorInvalidValue;
  const size_t nblocks = (size_t)N * (K / 32);
  QUANT_DT(dt, hipLaunchKernelGGL((dequant_rows_mxfp4_kernel<DT>), dim3(quant_grid(nblocks, 256)),
                                  dim3(256), 0, st, (const uint8_t*)w4, (const uint8_t*)e8, nblocks,
                                  (uint16_t*)out16));
  return (int)hipGetLastError();
}
