// The MXFP4 weight format of the decode GEMV kernels (gemv_kernel.h), used by gemv_w4.hip,
// gemv_w4_mlp.hip and gemv_w4_head.hip, and by the kernel gemv_w4_x16.hip keeps for itself.
//
// Format (quant_mxfp4.hip writes it): w4[N, K/2] two e2m1 codes per byte (k even in the low
// nibble), e8[N, K/32] one e8m0 scale byte per 32 consecutive k,
// W[n, k] = 2^(e8[n, k/32] - 127) * e2m1(code).  K % 32 == 0.
//
// A lane's 16-byte chunk carries 32 k values — exactly one scale block — so each chunk
// comes with one scale byte per row (a wave's 64 chunks read 64 consecutive bytes of e8),
// requested together with the chunk.  The convert applies the block scale
// (v_cvt_scalef32_pk_f32_fp4: two codes and the scale per instruction), so the packed f32x2
// accumulators hold scaled products and the epilogues are those of the 16-bit format.
#pragma once
#include "gemv_kernel.h"
#include "mxfp4.h"

namespace cake {

struct W4 {
  static constexpr int kFmt = 2, kKinds = 4, kLog2 = 5, kPad32 = 2048, kPad16 = 2048;
  // A row is K / 32 chunks: 8B's K = 4096 is 2 per lane, 70B's K = 8192 is 4, the down
  // projections 7 and 14.  So the prefetch depths are PF in {0, 2, 4} chunks per row per
  // lane (2 = the whole row of an 8B hidden-width projection, 4 = of a 70B one) and U in
  // {1, 2, 4} for what follows it.
  static constexpr int kU[3] = {1, 2, 4}, kPF[2] = {4, 2};
  static constexpr bool kStrict = true, kRowScale = false;
  // The x row is kept in LDS in a permuted order, as W8::perm32 does for the fp8 kernels.
  // A lane's chunk is 32 consecutive values: 128 bytes of f32 or 64 bytes of 16-bit.
  // ds_read_b128 serves 16 lanes at a time over a 256-byte bank row, so a 128-byte lane
  // stride is an 8-way conflict and a 64-byte one 4-way.  Within every block of 64 chunks
  // (2048 values) the j-th 16-byte word of chunk l sits at word index j * 64 + l (8 words
  // per chunk in f32, 4 in 16-bit): each read of a lane is then contiguous across the wave.
  // LDS holds K rounded up to 2048 values.
  static __device__ __forceinline__ int perm32(int i) {  // i % 4 == 0: a float4's first float
    return (i & ~2047) | (((i >> 2) & 7) << 8) | (((i & 2047) >> 5) << 2);
  }
  static __device__ __forceinline__ int perm16(int i) {  // i % 8 == 0: a uint4's first value
    return (i & ~2047) | (((i >> 3) & 3) << 9) | (((i & 2047) >> 5) << 3);
  }
  // the deepest prefetch <= pf that the row fills: PF 4 on a 128-chunk row runs as 2, and
  // any depth as 0 when the row is shorter than 128 chunks
  static int prefetch(int pf, int K) {
    const int nch = K >> kLog2;
    return (pf >= 4 && nch >= 256) ? 4 : ((pf >= 2 && nch >= 128) ? 2 : 0);
  }
  using Acc = f32x2_t;
  static __device__ __forceinline__ Acc zero() { return {0.f, 0.f}; }
  static __device__ __forceinline__ float total(Acc a) { return a.x + a.y; }
  struct Mat {
    const uint8_t* w;   // [N, K/2] codes
    const uint8_t* e8;  // [N, K/32] scale bytes
  };
  static __device__ __forceinline__ Mat pick(const Mat& q, const Mat& k, const Mat& v, int kind) {
    return {pick3(q.w, k.w, v.w, kind), pick3(q.e8, k.e8, v.e8, kind)};
  }
  // the code and scale rows of a pair
  struct Rows {
    const uint4 *a, *b;
    const uint8_t *ea, *eb;
  };
  static __device__ __forceinline__ Rows rows(const Mat& ma, size_t ra, const Mat& mb, size_t rb,
                                              int K) {
    const size_t rowb = (size_t)K >> 1, rowe = (size_t)K >> 5;
    return {reinterpret_cast<const uint4*>(ma.w + ra * rowb),
            reinterpret_cast<const uint4*>(mb.w + rb * rowb), ma.e8 + ra * rowe,
            mb.e8 + rb * rowe};
  }
  // a chunk of both rows and its two scale bytes
  struct Chunk {
    uint4 a, b;
    uint32_t ea, eb;
  };
  template <bool NT> static __device__ __forceinline__ Chunk load(const Rows& r, int c) {
    if constexpr (NT) return {ld_nt16(r.a + c), ld_nt16(r.b + c), r.ea[c], r.eb[c]};
    else return {r.a[c], r.b[c], r.ea[c], r.eb[c]};
  }
  // 8 x values of a chunk: those of code dword D (k = 8 D .. 8 D + 7)
  template <int DT, bool XF32, int D>
  static __device__ __forceinline__ void load_x8(const void* xs, int chunk, float* o) {
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
  static __device__ __forceinline__ void fma_dword(const float* xv, uint32_t wa, uint32_t wb,
                                                   float sa, float sb, Acc& acc_a, Acc& acc_b) {
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
  // one chunk of both rows: 32 k values
  template <int DT, bool XF32>
  static __device__ __forceinline__ void fma(const void* xs, int chunk, const Chunk& v, Acc& acc_a,
                                             Acc& acc_b) {
    const float sa = e8m0_to_f32(v.ea), sb = e8m0_to_f32(v.eb);
    float xv[8];
    load_x8<DT, XF32, 0>(xs, chunk, xv);
    fma_dword(xv, v.a.x, v.b.x, sa, sb, acc_a, acc_b);
    load_x8<DT, XF32, 1>(xs, chunk, xv);
    fma_dword(xv, v.a.y, v.b.y, sa, sb, acc_a, acc_b);
    load_x8<DT, XF32, 2>(xs, chunk, xv);
    fma_dword(xv, v.a.z, v.b.z, sa, sb, acc_a, acc_b);
    load_x8<DT, XF32, 3>(xs, chunk, xv);
    fma_dword(xv, v.a.w, v.b.w, sa, sb, acc_a, acc_b);
  }
};

}  // namespace cake
