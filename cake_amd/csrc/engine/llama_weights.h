// Resident weight matrices of the native Llama engine (llama_engine.cpp): one value type for
// an [N, K] matrix in any weight format, and the one place that picks a decode GEMV's entry
// point by format.  The engine holds Mats and calls the dispatchers below; nothing else in
// it names a _w8 / _w4 / _p13 / quantiser entry point or does a sub-matrix's offset arithmetic.
#pragma once

#include <string>

#include "../kernels/cake_kernels.h"
#include "engine_util.h"

namespace cake {

// CakeEngineOpts.weight_fmt / head_fmt
enum WeightFmt : int { kFmt16 = 0, kFmtFp8 = 1, kFmtMxfp4 = 2 };

// per format: the multiple every matrix width K must be, the name in refusals and the name in
// the open banner (16-bit: the model dtype's instead)
struct FmtFacts { int multiple; const char *name, *banner; };
inline const FmtFacts& fmt_facts(int fmt) {
  static const FmtFacts f[3] = {{1, "", ""}, {16, "fp8", "fp8 e4m3"}, {32, "mxfp4", "mxfp4"}};
  return f[fmt];
}
// bytes of an [N, K] matrix's data (16-bit rows / e4m3 codes / two e2m1 codes per byte) and of
// its side data (none / one f32 scale per row / one e8m0 byte per 32 elements of a row)
inline size_t fmt_code_bytes(int fmt, size_t N, size_t K) {
  return fmt == kFmtFp8 ? N * K : fmt == kFmtMxfp4 ? N * K / 2 : N * K * 2;
}
inline size_t fmt_side_bytes(int fmt, size_t N, size_t K) {
  return fmt == kFmtFp8 ? N * 4 : fmt == kFmtMxfp4 ? N * K / 32 : 0;
}

struct P13Mat {  // one matrix packed by cake_pack13_rows: one allocation, three parts
  uint8_t* planes = nullptr;
  int* hdr = nullptr;
  uint16_t* raw = nullptr;  // null: no raw rows
};

// the GEMV family that reads a Mat, and its suffix in the k_check labels
enum GemvPath : int { kPath16 = 0, kPathW8 = 1, kPathW4 = 2, kPathP13 = 3 };

// One resident [N, K] matrix.  kFmt16: w the 16-bit rows, and p13 (planes non-null) the packed
// twin the decode GEMVs stream instead: only bf16 weights on one rank have one.  kFmtFp8: w
// the e4m3 codes [N, K], scale the f32 row scales [N].  kFmtMxfp4: w the packed e2m1 codes
// [N, K/2], e8 the e8m0 block-scale bytes [N, K/32].
struct Mat {
  int fmt = kFmt16;
  size_t N = 0, K = 0;
  void* w = nullptr;
  float* scale = nullptr;
  uint8_t* e8 = nullptr;
  P13Mat p13;

  // rows [r0, r0 + n) (n = 0: to the end) as a matrix of their own: q | k | v and gate | up
  // are packed as one matrix.  p13.raw is a table for the whole matrix and does not move.
  Mat rows(size_t r0, size_t n = 0) const {
    Mat s = *this;
    s.N = n ? n : N - r0;
    s.w = static_cast<uint8_t*>(w) + fmt_code_bytes(fmt, r0, K);
    if (scale) s.scale = scale + r0;
    if (e8) s.e8 = e8 + r0 * (K / 32);
    if (p13.planes) {
      s.p13.planes = p13.planes + r0 * (K / 8 * 13);
      s.p13.hdr = p13.hdr + r0;
    }
    return s;
  }
  // what the matrix adds to the engine's weight bytes (the packed twin is counted apart)
  size_t bytes() const { return fmt_code_bytes(fmt, N, K) + fmt_side_bytes(fmt, N, K); }
  GemvPath path() const {
    return fmt == kFmt16 ? (p13.planes ? kPathP13 : kPath16) : static_cast<GemvPath>(fmt);
  }
};

// k_check with the label of the entry point that ran for m: what + "", "_w8", "_w4", "_p13"
inline void k_check(int rc, const char* what, const Mat& m) {
  static const char* const suffix[4] = {"", "_w8", "_w4", "_p13"};
  if (rc != 0) k_check(rc, (std::string(what) + suffix[m.path()]).c_str());
}

// ---- the decode GEMV families: each takes its C entry point's arguments with the weight
// pointers replaced by the Mat and runs the entry point of the Mat's format (16-bit with a
// packed twin: the P13 one; without, as on a tensor-parallel rank: the plain one).  t... are
// the arguments after the weights, the same in all four forms.

// q | k | v + RoPE + KV write (t: inv_freq, pos, q_out, kcache, vcache, S, st, kv_fmt)
template <class... T>
int qkv_rope(int dt, const float* resid, const void* norm_w, float eps, const Mat& m, int K, int nh,
             int nkv, int hd, T... t) {
  const Mat k = m.rows((size_t)nh * hd), v = m.rows((size_t)(nh + nkv) * hd);
  const P13Mat &pq = m.p13, &pk = k.p13, &pv = v.p13;
  switch (m.path()) {
    case kPathW8:
      return cake_qkv_rope_w8_kvf(dt, resid, norm_w, eps, m.w, k.w, v.w, m.scale, k.scale, v.scale,
                                  K, nh, nkv, hd, t...);
    case kPathW4:
      return cake_qkv_rope_w4_kvf(dt, resid, norm_w, eps, m.w, k.w, v.w, m.e8, k.e8, v.e8, K, nh,
                                  nkv, hd, t...);
    case kPathP13:
      return cake_qkv_rope_p13_kvf(dt, resid, norm_w, eps, pq.planes, pk.planes, pv.planes, pq.hdr,
                                   pk.hdr, pv.hdr, pq.raw, pk.raw, pv.raw, K, nh, nkv, hd, t...);
    default: return cake_qkv_rope_kvf(dt, resid, norm_w, eps, m.w, k.w, v.w, K, nh, nkv, hd, t...);
  }
}

// out (+)= m . x for a 16-bit x: o_proj and down_proj (t: K, N, out, accumulate, st)
template <class... T>
int gemv_x16(int dt, const void* x, const Mat& m, T... t) {
  switch (m.path()) {
    case kPathW8: return cake_gemv_x16_w8(dt, x, m.w, m.scale, t...);
    case kPathW4: return cake_gemv_x16_w4(dt, x, m.w, m.e8, t...);
    case kPathP13: return cake_gemv_x16_p13(dt, x, m.p13.planes, m.p13.hdr, m.p13.raw, t...);
    default: return cake_gemv_x16(dt, x, m.w, t...);
  }
}

// act = silu(gate . x) * (up . x), x = rms_norm(resid) (t: act, st); m is the packed [2 I, K]
template <class... T>
int swiglu(int dt, const float* resid, const void* norm_w, float eps, const Mat& m, int K, int I,
           T... t) {
  const Mat u = m.rows((size_t)I);
  switch (m.path()) {
    case kPathW8:
      return cake_swiglu_w8(dt, resid, norm_w, eps, m.w, u.w, m.scale, u.scale, K, I, t...);
    case kPathW4: return cake_swiglu_w4(dt, resid, norm_w, eps, m.w, u.w, m.e8, u.e8, K, I, t...);
    case kPathP13:
      return cake_swiglu_p13(dt, resid, norm_w, eps, m.p13.planes, u.p13.planes, m.p13.hdr,
                             u.p13.hdr, m.p13.raw, u.p13.raw, K, I, t...);
    default: return cake_swiglu(dt, resid, norm_w, eps, m.w, u.w, K, I, t...);
  }
}

// out = m . rms_norm(resid) in f32, the lm_head (t: K, N, out, st)
template <class... T>
int gemv_norm_f32(int dt, const float* resid, const void* norm_w, float eps, const Mat& m, T... t) {
  const P13Mat& p = m.p13;
  switch (m.path()) {
    case kPathW8: return cake_gemv_norm_f32_w8(dt, resid, norm_w, eps, m.w, m.scale, t...);
    case kPathW4: return cake_gemv_norm_f32_w4(dt, resid, norm_w, eps, m.w, m.e8, t...);
    case kPathP13:
      return cake_gemv_norm_f32_p13(dt, resid, norm_w, eps, p.planes, p.hdr, p.raw, t...);
    default: return cake_gemv_norm_f32(dt, resid, norm_w, eps, m.w, t...);
  }
}

// the fused greedy tail: lm_head + penalty + argmax + next embedding row (t: K, N, out, ...)
template <class... T>
int head_select(int dt, const float* resid, const void* norm_w, float eps, const Mat& m, T... t) {
  const P13Mat& p = m.p13;
  switch (m.path()) {
    case kPathW8: return cake_head_select_w8(dt, resid, norm_w, eps, m.w, m.scale, t...);
    case kPathW4: return cake_head_select_w4(dt, resid, norm_w, eps, m.w, m.e8, t...);
    case kPathP13:
      return cake_head_select_p13(dt, resid, norm_w, eps, p.planes, p.hdr, p.raw, t...);
    default: return cake_head_select(dt, resid, norm_w, eps, m.w, t...);
  }
}

// rows16 [N, K] in dt -> m's codes and side data (allocated by the caller; not for kFmt16)
inline int quantise(const Mat& m, const void* rows16, int dt, hipStream_t st) {
  return m.fmt == kFmtFp8
             ? cake_quant_rows_fp8(dt, rows16, (int)m.N, (int)m.K, m.w, m.scale, st)
             : cake_quant_rows_mxfp4(dt, rows16, (int)m.N, (int)m.K, m.w, m.e8, st);
}

// rows [r0, r0 + n) of m as 16-bit rows in dt: the resident rows themselves, or the codes
// widened into scratch (room for n K values; stream order keeps its uses apart)
inline const void* dense16(const Mat& m, size_t r0, size_t n, void* scratch, int dt,
                           hipStream_t st) {
  const Mat s = m.rows(r0, n);
  if (s.fmt == kFmt16) return s.w;
  const bool f8 = s.fmt == kFmtFp8;
  k_check(f8 ? cake_dequant_rows_fp8(dt, s.w, s.scale, (int)n, (int)s.K, scratch, st)
             : cake_dequant_rows_mxfp4(dt, s.w, s.e8, (int)n, (int)s.K, scratch, st),
          f8 ? "dequant_rows_fp8" : "dequant_rows_mxfp4");
  return scratch;
}

}  // namespace cake
