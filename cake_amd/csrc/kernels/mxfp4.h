// MXFP4 decode helpers shared by quant_mxfp4.hip and the MXFP4 GEMV format (gemv_w4_kernel.h).
#pragma once
#include "common.h"

namespace cake {

typedef float f32x2_t __attribute__((ext_vector_type(2)));

// the e8m0 scale byte (1..254) as f32: 2^(code - 127), exact
__device__ __forceinline__ float e8m0_to_f32(uint32_t code) { return __uint_as_float(code << 23); }

// the two e2m1 codes of byte SEL of a dword, times the power-of-two `scale`
// (v_cvt_scalef32_pk_f32_fp4): [0] = the low nibble (element 2i), [1] = the high nibble
template <int SEL> __device__ __forceinline__ f32x2_t fp4x2_to_f32(uint32_t w, float scale) {
  return __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, scale, SEL);
}

}  // namespace cake
