// What crosses the translation units of the GEMM family (internal; the library is built with -fvisibility=hidden, nothing here is exported):
// the launch arguments gemm.hip fills, the one launcher each kernel unit defines, and the host helpers they share.
#pragma once
#include "devit_common.h"

struct LnBwdArgs;   // ln_rows.h

namespace devit_gemm {

constexpr int BK = 64;

// Internal epilogue kind behind devit_epilogue_kind's last value: the split-K epilogue of deterministic mode (gemm.hip rewrites ATOMIC_F32 to it;
// no caller passes it): partial tiles by plain stores into the workspace instead of fp32 atomics into the destination.
constexpr int DEVIT_EPI_DET_F32 = DEVIT_EPI_STORE_F32 + 1;

// n / d for 0 <= n < 2^31 by multiply-shift (Granlund-Montgomery round-up): three SALU ops instead of the
// float-reciprocal sequence hipcc emits for a scalar division.  Host-initialised.
struct FastDiv {
  unsigned mul, shift;
  int d;
};
__host__ inline FastDiv make_fastdiv(int d) {
  FastDiv f;
  f.d = d;
  unsigned s = 0;
  while ((1ll << s) < d) ++s;
  f.shift = 31 + s;
  f.mul = (unsigned)(((1ull << f.shift) / (unsigned long long)d) + 1ull);
  return f;
}

// One launch of gemm_kernel / gemm4_kernel / gemmfr_kernel (their argument type GemmArgs, gemm_device.h, is this and nothing more)
struct GemmParams {
  const __bf16* A;
  const __bf16* B;
  int lda, ldb;
  int a_group, a_skip, b_group, b_skip;
  long long a_bs, b_bs;
  int M, N, K;
  int tiles_m, tiles_n, split_k, total_tiles;
  FastDiv d_per_z, d_chunk, d_gn, d_last, d_split;   // tiles per z-slice, per n-chunk; chunk widths; split_k
  int gn;  // n-tiles per L2 chunk: tiles are ordered chunk-major, then m, then n inside the chunk
  devit_epilogue ep;
};

// The launchers: `grid` workgroups of the persistent kernel the unit holds, instantiated for g.ep.kind (and the operand layouts `variant` =
// 2 * (A k-major) + (B k-major), 16-bit type g.ep.dtype16); a pair that is not instantiated is DEVIT_ERR_ARG, never another kernel.
int launch_gemm_tile128(const GemmParams& g, int variant, unsigned grid, hipStream_t s);   // gemm_tile128.hip: gemm_kernel, 128x128 tiles
int launch_gemm_tile256(const GemmParams& g, int variant, unsigned grid, hipStream_t s);   // gemm_tile256.hip: gemm_kernel, 256x256 ping-pong
int launch_gemm4(const GemmParams& g, unsigned grid, hipStream_t s);                       // gemm4.hip: gemm4_kernel
int launch_gemmfr(const GemmParams& g, const LnBwdArgs* ln, unsigned grid, hipStream_t s); // gemmfr.hip: gemmfr_kernel; ln: the fused LayerNorm backward

// gemm.hip
int reserved_cus();                          // CUs the persistent grids leave free (devit_set_reserved_cus / DEVIT_RESERVE_CUS)
int cu_count();                              // 0: the query failed
long long persistent_grid(int cus, int occ); // workgroups of a persistent grid with `occ` of them per CU
int gemm_force();                            // DEVIT_GEMM_FORCE
inline bool aligned16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

// Launch KERNEL with LDS bytes of dynamic LDS (more than a kernel gets by default: the limit is raised once per kernel).
template <auto KERNEL, int LDS, typename ARGS>
int launch_kernel(unsigned grid, unsigned block, hipStream_t s, const ARGS& args) {
  static bool attr = false;
  if (!attr) {
    hipError_t e = hipFuncSetAttribute((const void*)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, LDS);
    DEVIT_CHECK(e == hipSuccess, DEVIT_ERR_LAUNCH, "hipFuncSetAttribute: %s", hipGetErrorString(e));
    attr = true;
  }
  hipLaunchKernelGGL(KERNEL, dim3(grid), dim3(block), LDS, s, args);
  DEVIT_LAUNCH_CHECK();
  return DEVIT_OK;
}

}  // namespace devit_gemm
