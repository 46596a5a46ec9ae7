// C API, argument checks and the planner of the FP8 x FP8 MFMA GEMM (gemm_w8a8_kernel.h).
//
// Tile shapes (cfg), weight rows x tokens per 256-thread workgroup:
//   0: 128 x 128   wave 64 x 64, 16 accumulator blocks, 64 KB LDS (two workgroups per CU)
//   1:  64 x  64   wave 32 x 32,  4 accumulator blocks, 32 KB LDS
// (a 256 x 128 tile, one workgroup per CU, measured slower than 128 x 128 on every Llama
// projection shape and is not built.)
// No split-K: cake_gemm_w8a8_plan takes the 128 x 128 tile where its grid has more tiles
// than the 256 CUs and the 64 x 64 tile otherwise; at the Llama widths (N >= 4096) the small
// tile gives at least 512 workgroups from 512 tokens on, so no k-split is needed to fill
// the machine there.  Below 256 tokens the grid underfills and the K loop is serial per tile.
#include "gemm_w8a8_kernel.h"

using namespace cake;

namespace {

constexpr int kNumCfg = 2;
constexpr int kCfgBN[kNumCfg] = {128, 64};
constexpr int kCfgBM[kNumCfg] = {128, 64};
constexpr int kCUs = 256;

template <int DT, int EPI, int BN, int BM>
int launch(const W8A8Args& g0, hipStream_t st) {
  W8A8Args g = g0;
  g.tiles_m = (g.M + BM - 1) / BM;
  const long long tiles = (long long)g.tiles_m * ((g.Nv + BN - 1) / BN);
  if (tiles > 0x7fffffffLL) return (int)hipErrorInvalidValue;
  g.tiles = (int)tiles;
  g.xcd = tiles % 8 == 0;
  constexpr int lds = 2 * (BN + BM) * kW8BK;
  auto* fn = gemm_w8a8_kernel<DT, EPI, BN, BM>;
  static_assert(lds <= 65536, "a larger tile needs the dynamic LDS limit raised");
  hipLaunchKernelGGL(fn, dim3((unsigned)tiles), dim3(kW8Threads), lds, st, g);
  return (int)hipGetLastError();
}

template <int DT, int EPI>
int launch_cfg(int cfg, const W8A8Args& g, hipStream_t st) {
  switch (cfg) {
    case 0: return launch<DT, EPI, 128, 128>(g, st);
    case 1: return launch<DT, EPI, 64, 64>(g, st);
  }
  return (int)hipErrorInvalidValue;
}

template <int DT>
int launch_epi(int epi, int cfg, const W8A8Args& g, hipStream_t st) {
  switch (epi) {
    case kEpiStore: return launch_cfg<DT, kEpiStore>(cfg, g, st);
    case kEpiResid32: return launch_cfg<DT, kEpiResid32>(cfg, g, st);
    case kEpiSwiglu: return launch_cfg<DT, kEpiSwiglu>(cfg, g, st);
  }
  return (int)hipErrorInvalidValue;
}

bool aligned(const void* p, uintptr_t a) { return p && ((uintptr_t)p & (a - 1)) == 0; }

}  // namespace

CAKE_API int cake_gemm_w8a8_num_cfgs() { return kNumCfg; }

// The tile shape for [M tokens] x [Nv weight rows] (gated: both halves): 128 x 128 where that
// grid has more tiles than CUs, else 64 x 64 (measured on the 8B / 70B projection shapes:
// profiles/w8a8_gemm_shapes.jsonl).  K does not enter: there is no k-split.
CAKE_API int cake_gemm_w8a8_plan(int M, int Nv, int K) {
  (void)K;
  auto tiles = [&](int cfg) {
    return (long long)((Nv + kCfgBN[cfg] - 1) / kCfgBN[cfg]) * ((M + kCfgBM[cfg] - 1) / kCfgBM[cfg]);
  };
  return tiles(0) > kCUs ? 0 : 1;
}

// epi: kEpiStore (c), kEpiResid32 (r32 += ), kEpiSwiglu (w8 / sw hold 2 N rows, gate rows
// first; c[:, f] = silu(gate) * up).  cfg < 0: cake_gemm_w8a8_plan's choice.
CAKE_API int cake_gemm_w8a8(int dt, int epi, int cfg, const void* a8, long long lda,
                            const float* sa, const void* w8, long long ldb, const float* sw,
                            void* c, long long ldc, float* r32, long long ldr, int M, int N,
                            int K, hipStream_t st) {
  const bool gated = epi == kEpiSwiglu;
  if (epi != kEpiStore && epi != kEpiResid32 && epi != kEpiSwiglu) return (int)hipErrorInvalidValue;
  if (M < 1 || N < 1 || K < kW8BK || K % kW8BK) return (int)hipErrorInvalidValue;
  if (lda < K || ldb < K || lda % 16 || ldb % 16) return (int)hipErrorInvalidValue;
  if (!aligned(a8, 16) || !aligned(w8, 16) || !aligned(sa, 4) || !aligned(sw, 4))
    return (int)hipErrorInvalidValue;
  if (gated && N % 16) return (int)hipErrorInvalidValue;
  if ((long long)N * (gated ? 2 : 1) > 0x7fffffffLL) return (int)hipErrorInvalidValue;
  if (cfg >= kNumCfg) return (int)hipErrorInvalidValue;
  W8A8Args g{};
  if (epi == kEpiResid32) {
    if (!aligned(r32, 4) || ldr < N) return (int)hipErrorInvalidValue;
    g.vec = N % 4 == 0 && ldr % 4 == 0 && aligned(r32, 16);
  } else {
    if (!aligned(c, 2) || ldc < N) return (int)hipErrorInvalidValue;
    g.vec = N % 4 == 0 && ldc % 4 == 0 && aligned(c, 8);
  }
  g.a = (const uint8_t*)a8;
  g.b = (const uint8_t*)w8;
  g.sa = sa;
  g.sw = sw;
  g.c = (uint16_t*)c;
  g.r32 = r32;
  g.lda = lda; g.ldb = ldb; g.ldc = ldc; g.ldr = ldr;
  g.M = M; g.N = N; g.K = K;
  g.Nv = gated ? 2 * N : N;
  g.half = N;
  g.gated = gated ? 1 : 0;
  if (cfg < 0) cfg = cake_gemm_w8a8_plan(M, g.Nv, K);
  if (dt == kBF16) return launch_epi<kBF16>(epi, cfg, g, st);
  if (dt == kF16) return launch_epi<kF16>(epi, cfg, g, st);
  return (int)hipErrorInvalidValue;
}
