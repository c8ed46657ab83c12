// gemm_kernel on 128x128x64 tiles: four waves, two workgroups per CU (gemm_tile.h).
#include "gemm_tile.h"

int devit_gemm::launch_gemm_tile128(const GemmParams& g, int variant, unsigned grid, hipStream_t s) {
  return launch_gemm_tile<128, 128, 2, 2>(g, variant, grid, s);
}
