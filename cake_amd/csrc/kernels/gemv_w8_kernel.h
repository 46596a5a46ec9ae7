// The FP8 (OCP e4m3fn) weight format of the decode GEMV kernels (gemv_kernel.h), used by
// gemv_w8.hip, gemv_w8_mlp.hip, gemv_w8_x16.hip and gemv_w8_head.hip.
//
// Format: w8[N, K] one e4m3fn code per element, scale[N] f32 per output row,
// W[n, k] = scale[n] * fp8(w8[n, k])  (quant_fp8.hip writes it).  K % 16 == 0.
//
// A 16-byte chunk carries 16 k values; the dot product accumulates the unscaled codes in
// f32 (two codes per v_cvt_pk_f32_fp8, packed f32x2 accumulators) and the row scale
// multiplies the wave sum once in the epilogue (kRowScale).
#pragma once
#include "gemv_kernel.h"

namespace cake {

// two fp8 codes of a dword -> f32 (v_cvt_pk_f32_fp8; HI selects the upper 16 bits)
template <bool HI> __device__ __forceinline__ f32x2_t fp8x2_to_f32(uint32_t w) {
  return __builtin_amdgcn_cvt_pk_f32_fp8((int)w, HI);
}

struct W8 : PlainRows {
  static constexpr int kFmt = 1, kKinds = 4, kLog2 = 4, kPad32 = 1024, kPad16 = 1;
  // a row is half the bytes of its 16-bit twin — 8B's K = 4096 is 4 chunks per lane — so
  // the 16-bit tuning does not carry over: U in {1, 2, 4}, PF in {0, 2, 4}
  static constexpr int kU[3] = {1, 2, 4}, kPF[2] = {4, 2};
  static constexpr bool kStrict = true, kRowScale = true;
  // The f32 x row (RMSNorm output) is kept in LDS in a permuted order: a lane's chunk is 16
  // floats = 64 bytes, and 64-byte lane strides are a 4-way bank conflict on ds_read_b128
  // (16-lane groups over a 256-byte bank row).  Within every block of 64 chunks (1024
  // floats) the j-th float4 of chunk l sits at float4 index j * 64 + l, so each of a lane's
  // four reads is contiguous across the wave.  LDS holds K rounded up to 1024 floats.
  static __device__ __forceinline__ int perm32(int i) {  // i % 4 == 0: a float4's first float
    return (i & ~1023) | (((i >> 2) & 3) << 8) | (((i & 1023) >> 4) << 2);
  }
  static __device__ __forceinline__ int perm16(int i) { return i; }
  static int prefetch(int pf, int K) { return prefetch_if_filled<kLog2>(pf, K); }
  using Acc = f32x2_t;
  static __device__ __forceinline__ Acc zero() { return {0.f, 0.f}; }
  static __device__ __forceinline__ float total(Acc a) { return a.x + a.y; }
  struct Mat {
    const uint8_t* w;    // [N, K] e4m3fn
    const float* scale;  // [N] row scales
  };
  static __device__ __forceinline__ Mat pick(const Mat& q, const Mat& k, const Mat& v, int kind) {
    return {pick3(q.w, k.w, v.w, kind), pick3(q.scale, k.scale, v.scale, kind)};
  }
  static __device__ __forceinline__ Rows rows(const Mat& ma, size_t ra, const Mat& mb, size_t rb,
                                              int K) {
    return {reinterpret_cast<const uint4*>(ma.w + ra * K),
            reinterpret_cast<const uint4*>(mb.w + rb * K)};
  }
  // the 16 x values of a chunk
  template <int DT, bool XF32>
  static __device__ __forceinline__ void load_x16(const void* xs, int chunk, float* o) {
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
  template <int DT, bool XF32>
  static __device__ __forceinline__ void fma(const void* xs, int chunk, const Chunk& v, Acc& acc_a,
                                             Acc& acc_b) {
    float xv[16];
    load_x16<DT, XF32>(xs, chunk, xv);
    const uint32_t wa[4] = {v.a.x, v.a.y, v.a.z, v.a.w};
    const uint32_t wb[4] = {v.b.x, v.b.y, v.b.z, v.b.w};
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      const f32x2_t x01 = {xv[4 * d], xv[4 * d + 1]}, x23 = {xv[4 * d + 2], xv[4 * d + 3]};
      acc_a = __builtin_elementwise_fma(fp8x2_to_f32<false>(wa[d]), x01, acc_a);
      acc_b = __builtin_elementwise_fma(fp8x2_to_f32<false>(wb[d]), x01, acc_b);
      acc_a = __builtin_elementwise_fma(fp8x2_to_f32<true>(wa[d]), x23, acc_a);
      acc_b = __builtin_elementwise_fma(fp8x2_to_f32<true>(wb[d]), x23, acc_b);
    }
  }
};

}  // namespace cake
