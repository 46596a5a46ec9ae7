// P13: a lossless 13-bit packing of bf16 weights for the decode GEMV kernels (gemv_kernel.h),
// used by gemv_p13.hip, gemv_p13_mlp.hip, gemv_p13_head.hip and written by pack13.hip.
//
// Format.  A bf16 word is w = s(1) e(8) m(7); h = e >> 1 (the exponent's upper 7 bits),
// L = w & 0xff (the exponent's last bit and the mantissa, stored as it is).  Per row:
// top = max h, base = top - 15 (signed).  Per value: code = h ? h - base : 0 (1..15; 0 keeps
// h == 0, whose low byte carries +-0 and the denormals), stored as L (8) + s (1) + code (4).
// Decoding  h = code ? base + code : 0,  w = s << 15 | h << 8 | L  gives back every bit
// pattern.  A row with a value of 0 < h <= base (a magnitude ~30 binades under the row's top)
// is not representable: it stays raw 16-bit in a side table, and so does the other row of
// its pair (the packer knows the pairing: PackKind), so a wave decides once per pair.
//
// Layout.  K % 2048 == 0.  A row is K / 2048 tiles of 3328 bytes; a tile is what one wave
// reads for 2048 values, lane l owning the 16-bit chunks l, l + 64, l + 128, l + 192 (8
// values each) of the tile — the values, and the order, lane l has under W16:
//   [   0, 1024)  uint4 per lane: low bytes of chunks 0, 1 (value e of chunk j: byte 8 j + e)
//   [1024, 2048)  uint4 per lane: low bytes of chunks 2, 3
//   [2048, 3072)  uint4 per lane: word j = the codes of chunk j, value e in nibble 2 e
//                 (e < 4) or 2 (e - 4) + 1
//   [3072, 3328)  one word per lane: the sign of value e of chunk j at bit 8 (e & 3) + 2 j +
//                 (e >> 2)
// The row header word hdr[row] = (slot + 1) << 8 | (base & 0xff): slot = the row's place in
// the raw table [nraw, K] (none: the upper bits are 0).  A raw row's planes are zero.
//
// The dot product rebuilds the eight values of every chunk a W16 lane would have loaded (as the
// f32 unpack8 makes of them) and runs W16::fma's fmaf chain over them in W16's order, so
// every output equals the W16 kernel's bit for bit.
#pragma once
#include "gemv_kernel.h"

namespace cake {

constexpr int kP13Tile = 2048;       // values per wave tile
constexpr int kP13TileBytes = 3328;  // 2048 * 13 / 8
// which rows the kernels pair (a raw row makes its partner raw): (2p, 2p + 1) — the 16-bit
// input GEMVs and the lm_head; (i, i + hd / 2) of a head — q | k | v; (j, j + N / 2) — gate | up
enum PackKind { kPackAdjacent = 0, kPackHeadHalves = 1, kPackGateUp = 2 };

__host__ __device__ inline int p13_partner(int kind, int r, int N, int hd) {
  if (kind == kPackHeadHalves) return r % hd < hd / 2 ? r + hd / 2 : r - hd / 2;
  if (kind == kPackGateUp) return r < N / 2 ? r + N / 2 : r - N / 2;
  return (r ^ 1) < N ? (r ^ 1) : r;
}

__device__ __forceinline__ uint32_t p13_base4(int hdr) {  // base (7 bits) in every byte
  return (uint32_t)(hdr & 0x7f) * 0x01010101u;
}

// the high bytes (sign | h) of chunk j's values 0..3 (hia) and 4..7 (hib): code the chunk's
// nibbles, sgn the lane's sign word, base4 = p13_base4
__device__ __forceinline__ void p13_high(uint32_t code, uint32_t sgn, int j, uint32_t base4,
                                         uint32_t& hia, uint32_t& hib) {
  const uint32_t ca = code & 0x0f0f0f0fu, cb = (code >> 4) & 0x0f0f0f0fu;
  // 0x7f in every byte whose code is not 0
  const uint32_t ta = (ca + 0x7f7f7f7fu) & 0x80808080u, tb = (cb + 0x7f7f7f7fu) & 0x80808080u;
  const uint32_t ha = ca + ((ta - (ta >> 7)) & base4), hb = cb + ((tb - (tb >> 7)) & base4);
  // (h & 0x7f) | sign << 7 per byte (v_bfi_b32): base + code wraps in 7 bits for base < 0
  const uint32_t sa = sgn << (7 - 2 * j), sb = sgn << (6 - 2 * j);
  hia = (ha & 0x7f7f7f7fu) | (sa & 0x80808080u);
  hib = (hb & 0x7f7f7f7fu) | (sb & 0x80808080u);
}

// the eight bf16 words of chunk j (lo0 / lo1: the low bytes of values 0..3 / 4..7), as the
// uint4 a W16 lane loads
__device__ __forceinline__ uint4 p13_decode8(uint32_t lo0, uint32_t lo1, uint32_t code,
                                             uint32_t sgn, int j, uint32_t base4) {
  uint32_t hia, hib;
  p13_high(code, sgn, j, base4, hia, hib);
  uint4 o;
  o.x = __builtin_amdgcn_perm(hia, lo0, 0x05010400u);
  o.y = __builtin_amdgcn_perm(hia, lo0, 0x07030602u);
  o.z = __builtin_amdgcn_perm(hib, lo1, 0x05010400u);
  o.w = __builtin_amdgcn_perm(hib, lo1, 0x07030602u);
  return o;
}

// the same eight values as f32, what unpack8<kBF16> makes of that uint4 (word << 16): one
// v_perm_b32 per value places low and high byte over two zero bytes
__device__ __forceinline__ void p13_decode8f(uint32_t lo0, uint32_t lo1, uint32_t code,
                                             uint32_t sgn, int j, uint32_t base4, float* o) {
  uint32_t hia, hib;
  p13_high(code, sgn, j, base4, hia, hib);
  o[0] = __uint_as_float(__builtin_amdgcn_perm(hia, lo0, 0x04000c0cu));
  o[1] = __uint_as_float(__builtin_amdgcn_perm(hia, lo0, 0x05010c0cu));
  o[2] = __uint_as_float(__builtin_amdgcn_perm(hia, lo0, 0x06020c0cu));
  o[3] = __uint_as_float(__builtin_amdgcn_perm(hia, lo0, 0x07030c0cu));
  o[4] = __uint_as_float(__builtin_amdgcn_perm(hib, lo1, 0x04000c0cu));
  o[5] = __uint_as_float(__builtin_amdgcn_perm(hib, lo1, 0x05010c0cu));
  o[6] = __uint_as_float(__builtin_amdgcn_perm(hib, lo1, 0x06020c0cu));
  o[7] = __uint_as_float(__builtin_amdgcn_perm(hib, lo1, 0x07030c0cu));
}

__device__ __forceinline__ uint32_t ld_nt4(const uint32_t* p) { return __builtin_nontemporal_load(p); }

struct P13 {
  static constexpr int kFmt = 3, kKinds = kNumKinds, kLog2 = 5, kPad32 = 1, kPad16 = 1;
  // a chunk is a lane's share of one tile: 32 values per row (four W16 chunks), 26 registers
  // per pair.  U 1 / 2 / 3 is W16's 4 / 8 / 12 (4 tiles in flight would need every VGPR);
  // prefetch 1 / 2 its 4 / 8
  static constexpr int kU[3] = {1, 2, 3}, kPF[2] = {2, 1};
  static constexpr bool kStrict = true, kRowScale = false, kRawRows = true, kBf16Only = true;
  // left alone the accumulating 16-bit-input GEMV of one tile in flight is scheduled into 176
  // VGPRs (2 waves per SIMD); asked for 3 it takes 164, without scratch (U 2 and 3 would spill)
  static constexpr int x16_waves(int U) { return U == 1 ? 3 : 1; }
  static __device__ __forceinline__ int perm32(int i) { return i; }
  static __device__ __forceinline__ int perm16(int i) { return i; }
  static int prefetch(int pf, int K) { return PlainRows::prefetch_if_filled<kLog2>(pf, K); }
  using Acc = float;
  static __device__ __forceinline__ Acc zero() { return 0.f; }
  static __device__ __forceinline__ float total(Acc a) { return a; }
  struct Mat {
    const uint8_t* planes;  // [N, K / 2048, 3328]
    const int* hdr;         // [N] row headers
    const uint16_t* raw;    // [nraw, K] the raw rows
  };
  static __device__ __forceinline__ Mat pick(const Mat& q, const Mat& k, const Mat& v, int kind) {
    return {pick3(q.planes, k.planes, v.planes, kind), pick3(q.hdr, k.hdr, v.hdr, kind),
            pick3(q.raw, k.raw, v.raw, kind)};
  }
  // The headers are requested here and only requested: nothing looks at them before the
  // pair's dot product starts (is_raw, fma), and run_pairs asks for a pair's rows one pair
  // ahead (the first pair's ahead of the x prologue), so they add no round trip.
  struct Rows {
    const uint8_t *a, *b;
    int ha, hb;  // as loaded (one address per wave)
    const uint16_t *rawa, *rawb;
  };
  static __device__ __forceinline__ Rows rows(const Mat& ma, size_t ra, const Mat& mb, size_t rb,
                                              int K) {
    const size_t rowb = (size_t)(K / kP13Tile) * kP13TileBytes;
    return {ma.planes + ra * rowb, mb.planes + rb * rowb, ma.hdr[ra], mb.hdr[rb], ma.raw, mb.raw};
  }
  static __device__ __forceinline__ bool is_raw(const Rows& r) {  // wave-uniform
    return (__builtin_amdgcn_readfirstlane(r.ha | r.hb) >> 8) != 0;
  }
  static __device__ __forceinline__ PlainRows::Rows raw_rows(const Rows& r, int K) {
    const int sa = __builtin_amdgcn_readfirstlane(r.ha) >> 8;
    const int sb = __builtin_amdgcn_readfirstlane(r.hb) >> 8;
    return {reinterpret_cast<const uint4*>(r.rawa + (size_t)(sa - 1) * K),
            reinterpret_cast<const uint4*>(r.rawb + (size_t)(sb - 1) * K)};
  }
  struct Chunk {
    uint4 la0, la1, ca, lb0, lb1, cb;
    uint32_t sa, sb;
    int ha, hb;  // the rows' headers, untouched until fma
  };
  template <bool NT> static __device__ __forceinline__ Chunk load(const Rows& r, int c) {
    const size_t t = (size_t)(c >> 6) * kP13TileBytes;
    const int l = c & 63;
    const uint4* pa = reinterpret_cast<const uint4*>(r.a + t) + l;
    const uint4* pb = reinterpret_cast<const uint4*>(r.b + t) + l;
    const uint32_t* qa = reinterpret_cast<const uint32_t*>(r.a + t + 3072) + l;
    const uint32_t* qb = reinterpret_cast<const uint32_t*>(r.b + t + 3072) + l;
    Chunk v;
    if constexpr (NT) {
      v.la0 = ld_nt16(pa); v.la1 = ld_nt16(pa + 64); v.ca = ld_nt16(pa + 128); v.sa = ld_nt4(qa);
      v.lb0 = ld_nt16(pb); v.lb1 = ld_nt16(pb + 64); v.cb = ld_nt16(pb + 128); v.sb = ld_nt4(qb);
    } else {
      v.la0 = pa[0]; v.la1 = pa[64]; v.ca = pa[128]; v.sa = *qa;
      v.lb0 = pb[0]; v.lb1 = pb[64]; v.cb = pb[128]; v.sb = *qb;
    }
    v.ha = r.ha;
    v.hb = r.hb;
    return v;
  }
  template <int DT, bool XF32>
  static __device__ __forceinline__ void fma(const void* xs, int chunk, const Chunk& v, Acc& acc_a,
                                             Acc& acc_b) {
    if constexpr (DT == kBF16) {  // (the entry points refuse f16)
      const int c16 = ((chunk >> 6) << 8) + (chunk & 63);  // the tile's first W16 chunk of the lane
      const uint32_t la[8] = {v.la0.x, v.la0.y, v.la0.z, v.la0.w, v.la1.x, v.la1.y, v.la1.z, v.la1.w};
      const uint32_t lb[8] = {v.lb0.x, v.lb0.y, v.lb0.z, v.lb0.w, v.lb1.x, v.lb1.y, v.lb1.z, v.lb1.w};
      const uint32_t ca[4] = {v.ca.x, v.ca.y, v.ca.z, v.ca.w};
      const uint32_t cb[4] = {v.cb.x, v.cb.y, v.cb.z, v.cb.w};
      const uint32_t base_a = p13_base4(v.ha), base_b = p13_base4(v.hb);
#pragma unroll
      for (int j = 0; j < 4; ++j) {  // W16::fma of the lane's chunk c16 + 64 j, value for value
        float xv[8], fa[8], fb[8];
        load_x8<DT, XF32>(xs, c16 + j * 64, xv);
        p13_decode8f(la[2 * j], la[2 * j + 1], ca[j], v.sa, j, base_a, fa);
        p13_decode8f(lb[2 * j], lb[2 * j + 1], cb[j], v.sb, j, base_b, fb);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          acc_a = fmaf(fa[e], xv[e], acc_a);
          acc_b = fmaf(fb[e], xv[e], acc_b);
        }
      }
    }
  }
};

// the refusals of every P13 entry point: bf16 only, whole tiles, planes and headers present
static inline bool p13_bad(int dt, int K, const void* planes, const void* hdr) {
  return dt != kBF16 || K < kP13Tile || K % kP13Tile != 0 || planes == nullptr || hdr == nullptr;
}

}  // namespace cake
