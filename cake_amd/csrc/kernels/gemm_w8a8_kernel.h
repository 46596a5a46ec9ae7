// FP8 x FP8 MFMA GEMM for the quantised prefill: e4m3fn activation codes with one f32 scale
// per token against the engine's resident e4m3fn projection codes with their f32 row
// scales (quant_fp8.hip), f32 accumulation on v_mfma_f32_16x16x128_f8f6f4.
//
//   Y[m, n] = epilogue( (sa[m] * sw[n]) * sum_k fp8(a8[m, k]) * fp8(w8[n, k]) )
//
// Orientation: the WEIGHT rows are the instruction's A operand (result rows) and the
// activation rows its B operand (result columns), so a lane's four accumulator registers are
// four consecutive output features of one token: one 8-byte 16-bit store, or one 16-byte
// f32 read-modify-write, per 16x16 block.
//
// Lane-to-k map: lane l supplies row (l & 15) of its operand and the 32 code bytes of k-group
// (l >> 4) in its eight operand registers.  Both operands use the same map, and the kernel
// feeds both from the same 32-byte slice of a 128-byte k-step, so the result does not depend
// on which k the hardware assigns to which byte (tests/test_w8a8_kernels_gpu.py pins the map
// with one-hot rows).  The block-scale operands are the e8m0 byte 127 (2^0) in every byte of
// the scale register, whichever byte the op_sel picks.
//
// Grid: one workgroup per tile, token tiles fastest, XCD-grouped (see the kernel).
//
// Staging: one k-step is 128 code bytes per row (as the bf16 kernel's 64-k step).  Every
// thread carries 16-byte chunks global -> registers -> LDS one step ahead of the MFMAs, two
// LDS buffers, one barrier per step.  LDS rows are 128 bytes with the 16-byte chunk index
// XORed with (row & 7): the eight rows that a group of lanes reads at one k-group fall in
// eight distinct bank groups.
#pragma once
#include "common.h"
#include "gemm_kernel.h"  // GemmEpi

namespace cake {

constexpr int kW8BK = 128;       // code bytes (= k) per step
constexpr int kW8Threads = 256;  // 4 waves, 2 (features) x 2 (tokens)

struct W8A8Args {
  const uint8_t* a;   // [M][lda] activation codes
  const uint8_t* b;   // [Nw][ldb] weight codes
  const float* sa;    // [M]
  const float* sw;    // [Nw]
  uint16_t* c;        // [M][ldc] 16-bit output (store, swiglu)
  float* r32;         // [M][ldr] f32 residual (resid32)
  long long lda, ldb, ldc, ldr;
  int M, N, K;        // N = output features; Nv = virtual weight rows
  int Nv, half;       // gated: Nv = 2 * half, half = N
  int gated;
  int vec;            // the output rows take aligned 4-feature vector accesses
  int tiles_m, tiles;  // token tiles; all tiles of the grid
  int xcd;             // tiles % 8 == 0: each XCD takes a contiguous eighth of the tile order
};

// virtual weight row -> weight row (gated: [16 gate rows | 16 up rows] per 32-row block)
__device__ __forceinline__ int w8_wrow(const W8A8Args& g, int v) {
  if (!g.gated) return v;
  const int blk = v >> 5, w = v & 31;
  return w < 16 ? blk * 16 + w : g.half + blk * 16 + (w - 16);
}

typedef int ci32x8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ cf32x4 w8_mfma(const ci32x8 a, const ci32x8 b, cf32x4 c) {
  // cbsz = blgp = 0: both operands e4m3; scales: e8m0 127 = 1.0
  return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, c, 0, 0, 0, 0x7f7f7f7f, 0,
                                                          0x7f7f7f7f);
}

__device__ __forceinline__ ci32x8 w8_frag(const uint8_t* lds, int o0, int o1) {
  const uint4 lo = *reinterpret_cast<const uint4*>(lds + o0);
  const uint4 hi = *reinterpret_cast<const uint4*>(lds + o1);
  ci32x8 f;
  f[0] = (int)lo.x; f[1] = (int)lo.y; f[2] = (int)lo.z; f[3] = (int)lo.w;
  f[4] = (int)hi.x; f[5] = (int)hi.y; f[6] = (int)hi.z; f[7] = (int)hi.w;
  return f;
}

// BN weight rows x BM tokens per workgroup; each wave (BN / 2) x (BM / 2)
template <int DT, int EPI, int BN, int BM>
__global__ __launch_bounds__(kW8Threads) void gemm_w8a8_kernel(W8A8Args g) {
  static_assert(EPI == kEpiStore || EPI == kEpiResid32 || EPI == kEpiSwiglu, "epilogue");
  static_assert(BN % 64 == 0 && BM % 64 == 0, "tile");
  constexpr bool GATED = EPI == kEpiSwiglu;
  constexpr int WN = BN / 2, WM = BM / 2, FN = WN / 16, FM = WM / 16;
  constexpr int CW = BN * 8 / kW8Threads, CX = BM * 8 / kW8Threads;  // chunks per thread
  constexpr int kBufBytes = (BN + BM) * kW8BK;
  extern __shared__ __attribute__((aligned(16))) uint8_t w8_smem[];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wn = wave & 1, wm = wave >> 1;
  // Tile order: token tiles fastest, so the workgroups in flight together share weight tiles
  // (the weights are the large operand: [N, K] against [T, K] with T <= a few thousand) and
  // the weights stream from memory once.  Workgroup ids go round the 8 XCDs; the remap gives
  // each XCD a contiguous run of the order, so the sharers of a weight tile share one L2.
  int id = blockIdx.x;
  if (g.xcd) id = (id & 7) * (g.tiles >> 3) + (id >> 3);
  const int tm = id % g.tiles_m, tn = id / g.tiles_m;
  const int n0 = tn * BN, m0 = tm * BM;

  // this thread's chunks of a step: chunk c = tid + 256 i -> row c >> 3, 16-byte piece c & 7
  const uint8_t* wsrc[CW];
  const uint8_t* xsrc[CX];
  int wdst[CW], xdst[CX];
#pragma unroll
  for (int i = 0; i < CW; ++i) {
    const int c = tid + kW8Threads * i, row = c >> 3, ch = c & 7;
    const int v = n0 + row;
    wsrc[i] = v < g.Nv ? g.b + (size_t)w8_wrow(g, v) * g.ldb + ch * 16 : nullptr;
    wdst[i] = row * kW8BK + ((ch ^ (row & 7)) << 4);
  }
#pragma unroll
  for (int i = 0; i < CX; ++i) {
    const int c = tid + kW8Threads * i, row = c >> 3, ch = c & 7;
    const int m = m0 + row;
    xsrc[i] = m < g.M ? g.a + (size_t)m * g.lda + ch * 16 : nullptr;
    xdst[i] = BN * kW8BK + row * kW8BK + ((ch ^ (row & 7)) << 4);
  }

  uint4 wreg[CW], xreg[CX];
  auto load_g = [&](int k0) {
#pragma unroll
    for (int i = 0; i < CW; ++i)
      wreg[i] = wsrc[i] ? *reinterpret_cast<const uint4*>(wsrc[i] + k0) : make_uint4(0, 0, 0, 0);
#pragma unroll
    for (int i = 0; i < CX; ++i)
      xreg[i] = xsrc[i] ? *reinterpret_cast<const uint4*>(xsrc[i] + k0) : make_uint4(0, 0, 0, 0);
  };
  auto write_lds = [&](uint8_t* buf) {
#pragma unroll
    for (int i = 0; i < CW; ++i) *reinterpret_cast<uint4*>(buf + wdst[i]) = wreg[i];
#pragma unroll
    for (int i = 0; i < CX; ++i) *reinterpret_cast<uint4*>(buf + xdst[i]) = xreg[i];
  };

  // fragment reads: row (lane & 15) of a 16-row block, 16-byte pieces 2 kg and 2 kg + 1
  const int r = lane & 15, kg = lane >> 4;
  const int f0 = r * kW8BK + (((2 * kg) ^ (r & 7)) << 4);
  const int f1 = r * kW8BK + (((2 * kg + 1) ^ (r & 7)) << 4);
  const int wbase = wn * WN * kW8BK, xbase = BN * kW8BK + wm * WM * kW8BK;

  cf32x4 acc[FN][FM];
#pragma unroll
  for (int i = 0; i < FN; ++i)
#pragma unroll
    for (int j = 0; j < FM; ++j) acc[i][j] = cf32x4{0.f, 0.f, 0.f, 0.f};

  const int nk = g.K / kW8BK;
  load_g(0);
  write_lds(w8_smem);
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const uint8_t* cur = w8_smem + (kt & 1) * kBufBytes;
    const bool more = kt + 1 < nk;
    if (more) load_g((kt + 1) * kW8BK);
    ci32x8 wf[FN];
#pragma unroll
    for (int i = 0; i < FN; ++i)
      wf[i] = w8_frag(cur + wbase + i * 16 * kW8BK, f0, f1);
#pragma unroll
    for (int j = 0; j < FM; ++j) {
      const ci32x8 xf = w8_frag(cur + xbase + j * 16 * kW8BK, f0, f1);
#pragma unroll
      for (int i = 0; i < FN; ++i) acc[i][j] = w8_mfma(wf[i], xf, acc[i][j]);
    }
    if (more) write_lds(w8_smem + ((kt + 1) & 1) * kBufBytes);
    __syncthreads();
  }

  // epilogue: acc[i][j][q] = virtual row n0 + wn WN + 16 i + 4 kg + q, token m0 + wm WM + 16 j + r
#pragma unroll
  for (int j = 0; j < FM; ++j) {
    const int m = m0 + wm * WM + j * 16 + r;
    if (m >= g.M) continue;
    const float sa = g.sa[m];
    if constexpr (GATED) {
#pragma unroll
      for (int i = 0; i < FN; i += 2) {
        const int v = n0 + wn * WN + i * 16 + kg * 4;  // gate rows; the up rows are v + 16
        if (v >= g.Nv) continue;
        const int f = (v >> 5) * 16 + (v & 15);
        float y[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float gt = (sa * g.sw[f + q]) * acc[i][j][q];
          const float up = (sa * g.sw[g.half + f + q]) * acc[i + 1][j][q];
          y[q] = silu(gt) * up;
        }
        uint16_t* dst = g.c + (size_t)m * g.ldc + f;
        if (g.vec) {
          *reinterpret_cast<uint2*>(dst) =
              make_uint2((uint32_t)from_f32<DT>(y[0]) | ((uint32_t)from_f32<DT>(y[1]) << 16),
                         (uint32_t)from_f32<DT>(y[2]) | ((uint32_t)from_f32<DT>(y[3]) << 16));
        } else {
#pragma unroll
          for (int q = 0; q < 4; ++q) dst[q] = from_f32<DT>(y[q]);
        }
      }
    } else {
#pragma unroll
      for (int i = 0; i < FN; ++i) {
        const int n = n0 + wn * WN + i * 16 + kg * 4;
        if (n >= g.N) continue;
        float y[4];
#pragma unroll
        for (int q = 0; q < 4; ++q)
          y[q] = n + q < g.N ? (sa * g.sw[n + q]) * acc[i][j][q] : 0.f;
        if constexpr (EPI == kEpiResid32) {
          float* dst = g.r32 + (size_t)m * g.ldr + n;
          if (g.vec) {
            float4 o = *reinterpret_cast<float4*>(dst);
            o.x += y[0]; o.y += y[1]; o.z += y[2]; o.w += y[3];
            *reinterpret_cast<float4*>(dst) = o;
          } else {
#pragma unroll
            for (int q = 0; q < 4; ++q)
              if (n + q < g.N) dst[q] += y[q];
          }
        } else {
          uint16_t* dst = g.c + (size_t)m * g.ldc + n;
          if (g.vec) {
            *reinterpret_cast<uint2*>(dst) =
                make_uint2((uint32_t)from_f32<DT>(y[0]) | ((uint32_t)from_f32<DT>(y[1]) << 16),
                           (uint32_t)from_f32<DT>(y[2]) | ((uint32_t)from_f32<DT>(y[3]) << 16));
          } else {
#pragma unroll
            for (int q = 0; q < 4; ++q)
              if (n + q < g.N) dst[q] = from_f32<DT>(y[q]);
          }
        }
      }
    }
  }
}

}  // namespace cake
