// Lock-step batched decode: the projections of up to 16 activation rows on one weight stream
// (gemv_rows_kernel.h) and the per-row twin of the decode QKV epilogue.
#include "gemv_rows_kernel.h"

namespace cake {

// per epilogue (store32, resid32, swiglu): row tiles per workgroup (an upper bound: halved
// while the grid would have fewer than kRowsMinGroups workgroups), k steps per trip, grid cap.
// Starting values, not yet swept on the device.
static RowsTune g_rows_tune[3] = {{2, 4, 4096}, {2, 4, 4096}, {2, 4, 4096}};

static int rows_kind(int epi) {
  return epi == kEpiStore32 ? 0 : epi == kEpiResid32 ? 1 : epi == kEpiSwiglu ? 2 : -1;
}

template <int DT, int EPI>
static int launch_rows(const RowsArgs& a0, const RowsTune& t, hipStream_t st) {
  RowsArgs a = a0;
  constexpr int kMaxR = EPI == kEpiSwiglu ? 2 : 4;  // 32 KiB of partial tiles at most
  int R = t.tiles < kMaxR ? t.tiles : kMaxR;
  auto groups = [&](int r) { return (a.N + 16 * r - 1) / (16 * r); };
  while (R > 1 && groups(R) < kRowsMinGroups) R >>= 1;
  a.ngroups = groups(R);
  const dim3 grid(a.ngroups < t.max_blocks ? a.ngroups : t.max_blocks), block(kRowsThreads);
#define CAKE_ROWS_RU(RV, UV) \
  hipLaunchKernelGGL((gemv_rows_kernel<DT, EPI, RV, UV>), grid, block, 0, st, a)
#define CAKE_ROWS_R(RV)       \
  do {                        \
    if (t.unroll == 2) CAKE_ROWS_RU(RV, 2); \
    else CAKE_ROWS_RU(RV, 4); \
  } while (0)
  if (R == 1) CAKE_ROWS_R(1);
  else if (R == 2) CAKE_ROWS_R(2);
  else if constexpr (kMaxR == 4) CAKE_ROWS_R(4);
#undef CAKE_ROWS_R
#undef CAKE_ROWS_RU
  return (int)hipGetLastError();
}

// q | k | v rows of M sequences after the store32 projection -> roped f32 q, roped k and plain
// v rounded once into row pos[m] of sequence m's own 16-bit cache ([nkv][S][hd] per layer, the
// layer at element layer_off of the bases in kbase[m] / vbase[m]).  The arithmetic is that of
// qkv_rope_kernel's epilogue.  One workgroup per row; a row whose position is outside [0, S)
// writes nothing.
template <int DT>
__global__ __launch_bounds__(256) void rope_kv_rows_kernel(
    const float* __restrict__ qkv, long long ldq, const int* __restrict__ pos_tab,
    const float* __restrict__ inv_freq, int nh, int nkv, int hd, int S, float* __restrict__ q_out,
    void* const* __restrict__ kbase, void* const* __restrict__ vbase, long long layer_off) {
  const int m = blockIdx.x, pos = pos_tab[m];
  if (pos < 0 || pos >= S) return;
  const int half = hd >> 1, nrope = (nh + nkv) * half, nv = nkv * hd;
  const float* row = qkv + (size_t)m * ldq;
  float* q = q_out + (size_t)m * nh * hd;
  uint16_t* kc = static_cast<uint16_t*>(kbase[m]) + layer_off;
  uint16_t* vc = static_cast<uint16_t*>(vbase[m]) + layer_off;
  for (int p = threadIdx.x; p < nrope + nv; p += blockDim.x) {
    if (p < nrope) {
      const int head = p / half, i = p - head * half;
      const float da = row[(size_t)head * hd + i], db = row[(size_t)head * hd + i + half];
      float s, c;
      sincosf((float)pos * inv_freq[i], &s, &c);
      const float oa = da * c - db * s, ob = da * s + db * c;
      if (head < nh) {
        q[(size_t)head * hd + i] = oa;
        q[(size_t)head * hd + i + half] = ob;
      } else {
        const size_t off = ((size_t)(head - nh) * S + pos) * hd + i;
        kc[off] = from_f32<DT>(oa);
        kc[off + half] = from_f32<DT>(ob);
      }
    } else {
      const int e = p - nrope, head = e / hd, i = e - head * hd;
      vc[((size_t)head * S + pos) * hd + i] = from_f32<DT>(row[(size_t)(nh + nkv + head) * hd + i]);
    }
  }
}

// RMSNorm of M f32 rows as two 16-bit terms: row m of out = y rounded (what cake_rmsnorm
// writes, bit for bit), row M + m = (y - that) rounded, y = x r w in f32.  The lm_head of the
// batched step multiplies both on one weight pass (gemv_rows over 2M rows) and adds the two
// f32 sums: the batch-1 head reads an f32 normalised row, and one 16-bit rounding of it moved
// the logits three times as far from an f32 model as either existing path sits.
template <int DT>
__global__ __launch_bounds__(256) void rmsnorm_split_kernel(const float* __restrict__ x,
                                                            const uint16_t* __restrict__ w,
                                                            float eps, int M, int H,
                                                            uint16_t* __restrict__ out) {
  __shared__ float red[16];
  const float* xr = x + (size_t)blockIdx.x * H;
  float ss = 0.f;
  for (int i = threadIdx.x * 4; i < H; i += blockDim.x * 4) {
    const float4 v = *reinterpret_cast<const float4*>(xr + i);
    ss += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
  }
  ss = block_sum(ss, red);
  const float r = rsqrtf(ss / (float)H + eps);
  uint16_t* hi = out + (size_t)blockIdx.x * H;
  uint16_t* lo = out + ((size_t)M + blockIdx.x) * H;
  for (int i = threadIdx.x * 4; i < H; i += blockDim.x * 4) {
    const float4 v = *reinterpret_cast<const float4*>(xr + i);
    const uint2 wv = *reinterpret_cast<const uint2*>(w + i);
    const float y[4] = {v.x * r * to_f32<DT>((uint16_t)(wv.x & 0xffff)),
                        v.y * r * to_f32<DT>((uint16_t)(wv.x >> 16)),
                        v.z * r * to_f32<DT>((uint16_t)(wv.y & 0xffff)),
                        v.w * r * to_f32<DT>((uint16_t)(wv.y >> 16))};
    uint16_t h[4], l[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      h[e] = from_f32<DT>(y[e]);
      l[e] = from_f32<DT>(y[e] - to_f32<DT>(h[e]));
    }
    *reinterpret_cast<uint2*>(hi + i) =
        make_uint2((uint32_t)h[0] | ((uint32_t)h[1] << 16), (uint32_t)h[2] | ((uint32_t)h[3] << 16));
    *reinterpret_cast<uint2*>(lo + i) =
        make_uint2((uint32_t)l[0] | ((uint32_t)l[1] << 16), (uint32_t)l[2] | ((uint32_t)l[3] << 16));
  }
}

}  // namespace cake

using namespace cake;

#define DISPATCH_DT(dt, ...)                       \
  do {                                             \
    if ((dt) == kBF16) { constexpr int DT = kBF16; __VA_ARGS__; } \
    else if ((dt) == kF16) { constexpr int DT = kF16; __VA_ARGS__; } \
    else return (int)hipErrorInvalidValue;         \
  } while (0)

// epi: kEpiStore32, kEpiResid32 or kEpiSwiglu; tiles 1, 2 or 4 (swiglu: 1 or 2); unroll 2 or 4
CAKE_API int cake_gemv_rows_set_tuning(int epi, int tiles, int unroll, int max_blocks) {
  const int kind = rows_kind(epi);
  if (kind < 0 || (tiles != 1 && tiles != 2 && tiles != 4) || (kind == 2 && tiles == 4) ||
      (unroll != 2 && unroll != 4) || max_blocks < 1)
    return (int)hipErrorInvalidValue;
  g_rows_tune[kind] = RowsTune{tiles, unroll, max_blocks};
  return 0;
}

CAKE_API int cake_gemv_rows_get_tuning(int epi, int* out3) {
  const int kind = rows_kind(epi);
  if (kind < 0 || !out3) return (int)hipErrorInvalidValue;
  out3[0] = g_rows_tune[kind].tiles;
  out3[1] = g_rows_tune[kind].unroll;
  out3[2] = g_rows_tune[kind].max_blocks;
  return 0;
}

CAKE_API int cake_gemv_rows(int dt, int epi, const void* x16, long long ldx, const void* w,
                            long long ldw, void* out, long long ldo, float* resid32, long long ldr,
                            int M, int N, int K, hipStream_t st) {
  const int kind = rows_kind(epi);
  if (kind < 0 || M < 1 || M > 16 || N < 1 || K < 32 || K % 32 != 0 || !x16 || !w) return (int)hipErrorInvalidValue;
  // 16-byte fragments: rows start on 16-byte boundaries
  if (ldx < K || ldw < K || ldx % 8 != 0 || ldw % 8 != 0 || (uintptr_t)x16 % 16 != 0 ||
      (uintptr_t)w % 16 != 0)
    return (int)hipErrorInvalidValue;
  if (epi == kEpiResid32 ? (!resid32 || ldr < N) : (!out || ldo < N)) return (int)hipErrorInvalidValue;
  const RowsArgs a{(const uint16_t*)x16, (const uint16_t*)w, out, resid32, ldx, ldw, ldo, ldr,
                   M, N, K, 0};
  const RowsTune t = g_rows_tune[kind];
  if (epi == kEpiStore32) DISPATCH_DT(dt, return (launch_rows<DT, kEpiStore32>(a, t, st)));
  if (epi == kEpiResid32) DISPATCH_DT(dt, return (launch_rows<DT, kEpiResid32>(a, t, st)));
  DISPATCH_DT(dt, return (launch_rows<DT, kEpiSwiglu>(a, t, st)));
  return 0;
}

CAKE_API int cake_rmsnorm_split_rows(int dt, const float* x, const void* w, float eps, int M, int H,
                                     void* out16, hipStream_t st) {
  if (M < 1 || M > 8 || H < 4 || H % 4 != 0 || !x || !w || !out16) return (int)hipErrorInvalidValue;
  DISPATCH_DT(dt, hipLaunchKernelGGL((rmsnorm_split_kernel<DT>), dim3(M), dim3(256), 0, st, x,
                                     (const uint16_t*)w, eps, M, H, (uint16_t*)out16));
  return (int)hipGetLastError();
}

CAKE_API int cake_rope_kv_rows(int dt, const float* qkv32, long long ldq, int M, const int* pos,
                               const float* inv_freq, int nh, int nkv, int hd, int S, float* q_out,
                               void* const* kbase, void* const* vbase, long long layer_off,
                               hipStream_t st) {
  if (M < 1 || M > 16 || nh < 1 || nkv < 1 || hd < 2 || hd % 2 != 0 || S < 1 || layer_off < 0 ||
      ldq < (long long)(nh + 2 * nkv) * hd || !qkv32 || !pos || !inv_freq || !q_out || !kbase ||
      !vbase)
    return (int)hipErrorInvalidValue;
  DISPATCH_DT(dt, hipLaunchKernelGGL((rope_kv_rows_kernel<DT>), dim3(M), dim3(256), 0, st, qkv32,
                                     ldq, pos, inv_freq, nh, nkv, hd, S, q_out, kbase, vbase,
                                     layer_off));
  return (int)hipGetLastError();
}
