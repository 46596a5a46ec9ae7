// 64-bit wave reductions and the ordered logit key shared by the log-sum-exp kernels
// (score.hip: rows of a logit block; logprob.hip: one decode row over several workgroups).
#pragma once

#include "common.h"

namespace cake {

// the head-select key of gemv_kernel.h: (ordered(x) << 32) | ~index, so the maximum is the
// largest logit with the lowest index at ties; keys of distinct indices are distinct
__device__ __forceinline__ unsigned int score_ordered(float f) {
  const unsigned int u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float score_unordered(unsigned int k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}
__device__ __forceinline__ unsigned long long score_key(float x, unsigned int index) {
  return ((unsigned long long)score_ordered(x) << 32) | (0xffffffffu - index);
}

// 64-bit values through the wave butterflies of common.h: both halves take the same DPP
// control / lane swap, so a lane always pairs with one partner's whole value
template <int CTRL> __device__ __forceinline__ unsigned long long dpp_u64(unsigned long long v) {
  const unsigned int lo = (unsigned int)__builtin_amdgcn_update_dpp(0, (int)(unsigned int)v, CTRL,
                                                                    0xF, 0xF, false);
  const unsigned int hi = (unsigned int)__builtin_amdgcn_update_dpp(
      0, (int)(unsigned int)(v >> 32), CTRL, 0xF, 0xF, false);
  return ((unsigned long long)hi << 32) | lo;
}
// the two values v_permlane{16,32}_swap pairs in this lane
template <int OFF>
__device__ __forceinline__ void swap_u64(unsigned long long v, unsigned long long& a,
                                         unsigned long long& b) {
  const int lo = (int)(unsigned int)v, hi = (int)(unsigned int)(v >> 32);
  if constexpr (OFF == 16) {
    const auto pl = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
    const auto ph = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
    a = ((unsigned long long)(unsigned int)ph[0] << 32) | (unsigned int)pl[0];
    b = ((unsigned long long)(unsigned int)ph[1] << 32) | (unsigned int)pl[1];
  } else {
    const auto pl = __builtin_amdgcn_permlane32_swap(lo, lo, false, false);
    const auto ph = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
    a = ((unsigned long long)(unsigned int)ph[0] << 32) | (unsigned int)pl[0];
    b = ((unsigned long long)(unsigned int)ph[1] << 32) | (unsigned int)pl[1];
  }
}

__device__ __forceinline__ unsigned long long umax64(unsigned long long a, unsigned long long b) {
  return a > b ? a : b;
}

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
  v = umax64(v, dpp_u64<kDppXor1>(v));
  v = umax64(v, dpp_u64<kDppXor2>(v));
  v = umax64(v, dpp_u64<kDppHalfMirror>(v));
  v = umax64(v, dpp_u64<kDppMirror>(v));
  unsigned long long a, b;
  swap_u64<16>(v, a, b);
  v = umax64(a, b);
  swap_u64<32>(v, a, b);
  return umax64(a, b);
}

__device__ __forceinline__ double wave_sum_f64(double d) {
  auto bits = [](double x) { return __builtin_bit_cast(unsigned long long, x); };
  auto dbl = [](unsigned long long x) { return __builtin_bit_cast(double, x); };
  d += dbl(dpp_u64<kDppXor1>(bits(d)));
  d += dbl(dpp_u64<kDppXor2>(bits(d)));
  d += dbl(dpp_u64<kDppHalfMirror>(bits(d)));
  d += dbl(dpp_u64<kDppMirror>(bits(d)));
  unsigned long long a, b;
  swap_u64<16>(bits(d), a, b);
  d = dbl(a) + dbl(b);
  swap_u64<32>(bits(d), a, b);
  return dbl(a) + dbl(b);
}

constexpr float kLog2e = 1.44269504088896340736f;

// exp(x - m) for m > -inf: v_exp_f32 of the f32 product (0 at x = -inf)
__device__ __forceinline__ double score_term(float x, float m) {
  return (double)__builtin_amdgcn_exp2f((x - m) * kLog2e);
}

}  // namespace cake
