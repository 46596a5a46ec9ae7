// P13 packer and unpacker: bf16 rows [N, K] <-> the lossless 13-bit planes of
// gemv_p13_kernel.h (format and layout there).  Packing is done once, when an engine opens;
// it is deterministic (the raw rows take their slots in row order) and runs on the device.
#include "gemv_p13_kernel.h"

namespace cake {

constexpr int kPackThreads = 256;

// tmp[row] = top | unrepresentable << 8: top = the row's largest h, unrepresentable = some
// value has 0 < h <= top - 15
__global__ __launch_bounds__(kPackThreads) void p13_scan_kernel(const uint16_t* __restrict__ w,
                                                                int K, int* __restrict__ tmp) {
  __shared__ int smax[kPackThreads / 64], smin[kPackThreads / 64];
  const uint4* p = reinterpret_cast<const uint4*>(w + (size_t)blockIdx.x * K);
  int hmax = 0, hmin = 128;  // hmin: the smallest h that is not 0
  for (int c = threadIdx.x; c < K / 8; c += kPackThreads) {
    const uint4 v = p[c];
    const uint32_t d[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int h = (int)((d[e >> 1] >> (16 * (e & 1) + 8)) & 0x7f);
      hmax = max(hmax, h);
      hmin = h ? min(hmin, h) : hmin;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    hmax = max(hmax, __shfl_xor(hmax, o));
    hmin = min(hmin, __shfl_xor(hmin, o));
  }
  if ((threadIdx.x & 63) == 0) {
    smax[threadIdx.x >> 6] = hmax;
    smin[threadIdx.x >> 6] = hmin;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int i = 1; i < kPackThreads / 64; ++i) {
      hmax = max(hmax, smax[i]);
      hmin = min(hmin, smin[i]);
    }
    const int unrep = hmin != 128 && hmin <= hmax - 15;
    tmp[blockIdx.x] = hmax | (unrep << 8);
  }
}

// one workgroup: a row is raw when it or its partner is unrepresentable; the raw rows take
// slots 0, 1, ... in row order; hdr (optional) gets the header words, *count the raw rows
__global__ __launch_bounds__(1024) void p13_assign_kernel(const int* __restrict__ tmp, int kind,
                                                          int N, int hd, int* __restrict__ hdr,
                                                          int* __restrict__ count) {
  __shared__ int scan[1024];
  int running = 0;
  for (int r0 = 0; r0 < N; r0 += 1024) {
    const int r = r0 + (int)threadIdx.x;
    int f = 0, top = 0;
    if (r < N) {
      const int t = tmp[r];
      top = t & 0xff;
      f = ((t | tmp[p13_partner(kind, r, N, hd)]) >> 8) & 1;
    }
    scan[threadIdx.x] = f;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {  // inclusive scan
      const int add = (int)threadIdx.x >= o ? scan[threadIdx.x - o] : 0;
      __syncthreads();
      scan[threadIdx.x] += add;
      __syncthreads();
    }
    if (r < N && hdr != nullptr) {
      const int slot = f ? running + scan[threadIdx.x] - 1 : -1;
      hdr[r] = ((slot + 1) << 8) | ((top - 15) & 0xff);
    }
    running += scan[1023];
    __syncthreads();
  }
  if (threadIdx.x == 0) *count = running;
}

// one thread per (row, tile, lane): the lane's 32 values of the tile
__global__ __launch_bounds__(kPackThreads) void p13_write_kernel(
    const uint16_t* __restrict__ w, size_t nlanes, int tiles, int K, const int* __restrict__ hdr,
    uint8_t* __restrict__ planes, uint16_t* __restrict__ raw) {
  for (size_t idx = (size_t)blockIdx.x * kPackThreads + threadIdx.x; idx < nlanes;
       idx += (size_t)gridDim.x * kPackThreads) {
    const int l = (int)(idx & 63);
    const size_t rt = idx >> 6, row = rt / tiles, t = rt % tiles;
    const int h = hdr[row], slot = (h >> 8) - 1, base = (int)(int8_t)(h & 0xff);
    const uint4* src = reinterpret_cast<const uint4*>(w + row * K + t * kP13Tile);
    uint32_t lo[8] = {0, 0, 0, 0, 0, 0, 0, 0}, code[4] = {0, 0, 0, 0}, sgn = 0;
    if (slot >= 0) {
      uint4* dst = reinterpret_cast<uint4*>(raw + (size_t)slot * K + t * kP13Tile);
#pragma unroll
      for (int j = 0; j < 4; ++j) dst[j * 64 + l] = src[j * 64 + l];
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint4 v = src[j * 64 + l];
        const uint32_t d[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const uint32_t x = (d[e >> 1] >> (16 * (e & 1))) & 0xffffu;
          const int h7 = (int)((x >> 8) & 0x7f);
          const uint32_t cd = h7 ? (uint32_t)(h7 - base) : 0u;
          lo[2 * j + (e >> 2)] |= (x & 0xffu) << (8 * (e & 3));
          code[j] |= cd << (4 * (e < 4 ? 2 * e : 2 * (e - 4) + 1));
          sgn |= (x >> 15) << (8 * (e & 3) + 2 * j + (e >> 2));
        }
      }
    }
    uint8_t* tp = planes + rt * kP13TileBytes;
    reinterpret_cast<uint4*>(tp)[l] = make_uint4(lo[0], lo[1], lo[2], lo[3]);
    reinterpret_cast<uint4*>(tp + 1024)[l] = make_uint4(lo[4], lo[5], lo[6], lo[7]);
    reinterpret_cast<uint4*>(tp + 2048)[l] = make_uint4(code[0], code[1], code[2], code[3]);
    reinterpret_cast<uint32_t*>(tp + 3072)[l] = sgn;
  }
}

__global__ __launch_bounds__(kPackThreads) void p13_unpack_kernel(
    const uint8_t* __restrict__ planes, const int* __restrict__ hdr,
    const uint16_t* __restrict__ raw, size_t nlanes, int tiles, int K, uint16_t* __restrict__ out) {
  for (size_t idx = (size_t)blockIdx.x * kPackThreads + threadIdx.x; idx < nlanes;
       idx += (size_t)gridDim.x * kPackThreads) {
    const int l = (int)(idx & 63);
    const size_t rt = idx >> 6, row = rt / tiles, t = rt % tiles;
    const int h = hdr[row], slot = (h >> 8) - 1;
    uint4* dst = reinterpret_cast<uint4*>(out + row * K + t * kP13Tile);
    if (slot >= 0) {
      const uint4* src = reinterpret_cast<const uint4*>(raw + (size_t)slot * K + t * kP13Tile);
#pragma unroll
      for (int j = 0; j < 4; ++j) dst[j * 64 + l] = src[j * 64 + l];
      continue;
    }
    const uint8_t* tp = planes + rt * kP13TileBytes;
    const uint4 l0 = reinterpret_cast<const uint4*>(tp)[l];
    const uint4 l1 = reinterpret_cast<const uint4*>(tp + 1024)[l];
    const uint4 cv = reinterpret_cast<const uint4*>(tp + 2048)[l];
    const uint32_t sgn = reinterpret_cast<const uint32_t*>(tp + 3072)[l];
    const uint32_t lo[8] = {l0.x, l0.y, l0.z, l0.w, l1.x, l1.y, l1.z, l1.w};
    const uint32_t code[4] = {cv.x, cv.y, cv.z, cv.w};
    const uint32_t base4 = p13_base4(h);
#pragma unroll
    for (int j = 0; j < 4; ++j)
      dst[j * 64 + l] = p13_decode8(lo[2 * j], lo[2 * j + 1], code[j], sgn, j, base4);
  }
}

static inline int pack_grid(size_t nlanes) {
  const size_t want = (nlanes + kPackThreads - 1) / kPackThreads;
  return (int)(want < 16384 ? want : 16384);
}

static inline bool pack_bad_shape(int kind, int N, int K, int hd) {
  if (N < 1 || K < kP13Tile || K % kP13Tile) return true;
  if (kind == kPackHeadHalves) return hd < 2 || hd % 2 || N % hd;
  if (kind == kPackGateUp) return N % 2 != 0;
  return kind != kPackAdjacent;
}

}  // namespace cake

using namespace cake;

// bytes of the packed form of [N, K] with nraw raw rows: planes | headers (padded to 16
// bytes) | raw rows, in that order in one allocation; -1: K is not whole tiles
CAKE_API long long cake_pack13_bytes(int N, int K, int nraw) {
  if (N < 1 || K < kP13Tile || K % kP13Tile || nraw < 0) return -1;
  return (long long)N * (K / kP13Tile) * kP13TileBytes + ((long long)N * 4 + 15) / 16 * 16 +
         (long long)nraw * K * 2;
}

// Pack bf16 rows16 [N, K]; kind: the PackKind of the kernel that will read them (hd: the
// head dimension of kPackHeadHalves).  Returns the number of raw rows (>= 0), or a negated
// hipError_t.  With planes, hdr and raw all null it only counts (the sizing pass); else
// planes [N, K / 2048, 3328] and hdr [N] are written, and raw [raw_cap, K] when there are
// raw rows (more than raw_cap: -hipErrorInvalidValue; hdr is already written then, planes
// and raw are not).  Synchronous.
CAKE_API int cake_pack13_rows(int kind, const void* rows16, int N, int K, int hd, void* planes,
                              int* hdr, void* raw, int raw_cap, hipStream_t st) {
  const bool count_only = planes == nullptr && hdr == nullptr && raw == nullptr;
  if (rows16 == nullptr || pack_bad_shape(kind, N, K, hd) || raw_cap < 0 ||
      (!count_only && (planes == nullptr || hdr == nullptr)))
    return -(int)hipErrorInvalidValue;
  int* tmp = nullptr;  // [N] scan results | the count
  hipError_t e = hipMalloc(&tmp, sizeof(int) * ((size_t)N + 1));
  if (e != hipSuccess) return -(int)e;
  const uint16_t* w = (const uint16_t*)rows16;
  int count = 0;
  hipLaunchKernelGGL(p13_scan_kernel, dim3(N), dim3(kPackThreads), 0, st, w, K, tmp);
  hipLaunchKernelGGL(p13_assign_kernel, dim3(1), dim3(1024), 0, st, tmp, kind, N, hd, hdr, tmp + N);
  e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(&count, tmp + N, sizeof(int), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e == hipSuccess && !count_only) {
    if (count > raw_cap || (count > 0 && raw == nullptr)) {
      e = hipErrorInvalidValue;
    } else {
      const int tiles = K / kP13Tile;
      const size_t nlanes = (size_t)N * tiles * 64;
      hipLaunchKernelGGL(p13_write_kernel, dim3(pack_grid(nlanes)), dim3(kPackThreads), 0, st, w,
                         nlanes, tiles, K, hdr, (uint8_t*)planes, (uint16_t*)raw);
      e = hipGetLastError();
      if (e == hipSuccess) e = hipStreamSynchronize(st);
    }
  }
  (void)hipFree(tmp);
  return e == hipSuccess ? count : -(int)e;
}

// the bf16 rows [N, K] back from their packed form
CAKE_API int cake_unpack13_rows(const void* planes, const int* hdr, const void* raw, int N, int K,
                                void* out16, hipStream_t st) {
  if (N < 1 || K < kP13Tile || K % kP13Tile || planes == nullptr || hdr == nullptr ||
      out16 == nullptr)
    return (int)hipErrorInvalidValue;
  const int tiles = K / kP13Tile;
  const size_t nlanes = (size_t)N * tiles * 64;
  hipLaunchKernelGGL(p13_unpack_kernel, dim3(pack_grid(nlanes)), dim3(kPackThreads), 0, st,
                     (const uint8_t*)planes, hdr, (const uint16_t*)raw, nlanes, tiles, K,
                     (uint16_t*)out16);
  return (int)hipGetLastError();
}
