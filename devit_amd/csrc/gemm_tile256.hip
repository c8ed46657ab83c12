// gemm_kernel on 256x256x64 tiles: eight waves, one workgroup per CU, the ping-pong schedule (gemm_tile.h).
#include "gemm_tile.h"

int devit_gemm::launch_gemm_tile256(const GemmParams& g, int variant, unsigned grid, hipStream_t s) {
  return launch_gemm_tile<256, 256, 2, 4>(g, variant, grid, s);
}
