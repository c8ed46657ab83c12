// Dropout p > 0 as passes of its own beside the GEMMs (nn.Dropout at models/de_vit.py:38,46 Mlp.drop, :72 attn_drop on the fp32 composite's P,
// :83 proj_drop, :173 pos_drop): the mask of dropout.h applied in place, or inside the residual + DropPath statement.  HBM-bound: every
// lane moves 16 bytes per access, one Philox call per four elements; rows are walked grid-stride.  Nothing here runs at p == 0.
#include "det.h"
#include "dropout.h"

namespace {

constexpr int CX = 64, RY = 4;   // a workgroup: 64 lanes x 16 bytes along a row (1 KiB), 4 rows

struct ApplyArgs {
  void* x;              // [rows][ld] bf16 or fp32, in place
  float* colsum;        // [cols] fp32, accumulated, or NULL
  int rows, cols, ld;
  long long pitch;      // of the LOGICAL tensor the mask is defined on (>= cols, % 4 == 0)
  DropKey d;
};

// F32 == false: 8 bf16 per lane (two Philox calls); true: 4 floats (one)
#define DROPOUT_APPLY_KERNEL dropout_apply_kernel
#define DROPOUT_APPLY_DET 0
#include "dropout_apply_kernel.inc"
#undef DROPOUT_APPLY_KERNEL
#undef DROPOUT_APPLY_DET
#define DROPOUT_APPLY_KERNEL dropout_apply_det_kernel
#define DROPOUT_APPLY_DET 1
#include "dropout_apply_kernel.inc"
#undef DROPOUT_APPLY_KERNEL
#undef DROPOUT_APPLY_DET

struct ResidualArgs {
  const float* x;       // [rows][cols]
  const float* y;       // [rows][cols]: the branch output (GEMM with the STORE_F32 epilogue)
  float* out;           // [rows][cols], may alias x
  const float* rowscale;
  int rows_per_scale, rows, cols;
  DropKey d;
};
__global__ __launch_bounds__(CX* RY) void dropout_residual_kernel(const ResidualArgs a) {
  const int c0 = (blockIdx.x * CX + threadIdx.x) * 4;
  if (c0 >= a.cols) return;
  for (int r = blockIdx.y * RY + threadIdx.y; r < a.rows; r += gridDim.y * RY) {
    const size_t o = (size_t)r * a.cols + c0;
    const f32x4 x = *(const f32x4*)(a.x + o), y = *(const f32x4*)(a.y + o);
    const float rs = a.rowscale ? a.rowscale[r / a.rows_per_scale] : 1.0f;
    const u32x4 w = drop_words(a.d, (unsigned long long)o);
    f32x4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = w[e] >= a.d.thr ? fmaf(rs, y[e] * a.d.s, x[e]) : x[e];
    *(f32x4*)(a.out + o) = v;
  }
}

struct MaskArgs {
  unsigned char* keep;  // [rows][cols]
  int rows, cols;
  long long pitch;
  DropKey d;
};
// debug / test entry point: the keep bytes themselves, one Philox call (four columns) per lane
__global__ __launch_bounds__(256) void dropout_mask_kernel(const MaskArgs a) {
  const int gpr = (a.cols + 3) >> 2;                        // column groups per row
  const long long total = (long long)a.rows * gpr;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int r = (int)(i / gpr), c0 = (int)(i % gpr) * 4;
    const u32x4 w = drop_words(a.d, (unsigned long long)r * (unsigned long long)a.pitch + (unsigned long long)c0);
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (c0 + e < a.cols) a.keep[(size_t)r * a.cols + c0 + e] = w[e] >= a.d.thr ? 1 : 0;
  }
}

bool al16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

// rows x (column chunks of one lane) -> grid: x covers the columns, y strides the rows with about eight workgroups per CU
dim3 row_grid(int rows, int lanes_x, int max_groups = 2048) {
  const int gx = (lanes_x + CX - 1) / CX;
  int gy = (rows + RY - 1) / RY;
  const int cap = max_groups / gx > 0 ? max_groups / gx : 1;
  if (gy > cap) gy = cap;
  return dim3(gx, gy > 0 ? gy : 1);
}

int check_site(const char* who, int site, int block, long long pitch, int cols) {
  DEVIT_CHECK(site >= 0 && site < DROP_SITES && block >= 0, DEVIT_ERR_ARG, "%s: site %d / block %d", who, site, block);
  DEVIT_CHECK(pitch >= cols && pitch % 4 == 0, DEVIT_ERR_ARG, "%s: pitch %lld must be a multiple of 4 and >= cols %d", who, pitch, cols);
  return DEVIT_OK;
}

}  // namespace

extern "C" int devit_dropout_mask(unsigned long long seed, int site, int block, unsigned thr, int rows, int cols, long long pitch,
                                  unsigned char* keep, void* stream) {
  DEVIT_CHECK(keep && rows > 0 && cols > 0, DEVIT_ERR_ARG, "devit_dropout_mask: bad argument");
  const int rc = check_site("devit_dropout_mask", site, block, pitch, cols);
  if (rc != DEVIT_OK) return rc;
  MaskArgs a{keep, rows, cols, pitch, drop_key(seed, site, block, thr, 1.0f)};
  const long long total = (long long)rows * ((cols + 3) / 4);
  const int grid = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
  hipLaunchKernelGGL(dropout_mask_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, a);
  DEVIT_LAUNCH_CHECK();
  return DEVIT_OK;
}

extern "C" int devit_dropout_apply(void* x, int is_f32, int rows, int cols, int ld, long long pitch, unsigned long long seed, int site,
                                   int block, unsigned thr, float scale_keep, float* colsum, void* stream) {
  DEVIT_CHECK(x && (is_f32 == 0 || is_f32 == 1) && rows > 0 && cols > 0, DEVIT_ERR_ARG, "devit_dropout_apply: bad argument");
  const int V = is_f32 ? 4 : 8;
  DEVIT_CHECK(cols % V == 0 && ld >= cols && ld % V == 0 && al16(x), DEVIT_ERR_ARG,
              "devit_dropout_apply: cols %d / ld %d must be multiples of %d (16-byte accesses) and x 16-byte aligned", cols, ld, V);
  const int rc = check_site("devit_dropout_apply", site, block, pitch, cols);
  if (rc != DEVIT_OK) return rc;
  ApplyArgs a{x, colsum, rows, cols, ld, pitch, drop_key(seed, site, block, thr, scale_keep)};
  // with column sums every workgroup ends in one atomic per column on the same words: one workgroup per CU then owns a long strip of rows
  // (2048 workgroups: 408 us for 78 MB at D = 384, all of it the atomics)
  const dim3 grid = row_grid(rows, cols / V, colsum ? 256 : 2048);
  if (colsum && grid.y > 1 && devit_det::on()) {   // deterministic mode (det.h): the strips' sums go to the workspace and are added to colsum in strip order
    float* ws = nullptr;
    const int rc = devit_det::workspace("devit_dropout_apply", (size_t)grid.y * cols * sizeof(float), &ws);
    if (rc != DEVIT_OK) return rc;
    a.colsum = ws;
    if (is_f32)
      hipLaunchKernelGGL(dropout_apply_det_kernel<true>, grid, dim3(CX, RY), 0, (hipStream_t)stream, a);
    else
      hipLaunchKernelGGL(dropout_apply_det_kernel<false>, grid, dim3(CX, RY), 0, (hipStream_t)stream, a);
    DEVIT_LAUNCH_CHECK();
    return devit_det::fold(ws, (int)grid.y, (size_t)cols, 1, cols, colsum, 0, 1, 0, (hipStream_t)stream);
  }
  if (is_f32)
    hipLaunchKernelGGL(dropout_apply_kernel<true>, grid, dim3(CX, RY), 0, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(dropout_apply_kernel<false>, grid, dim3(CX, RY), 0, (hipStream_t)stream, a);
  DEVIT_LAUNCH_CHECK();
  return DEVIT_OK;
}

extern "C" int devit_dropout_residual(const float* x, const float* y, float* x_out, const float* rowscale, int rows_per_scale, int rows,
                                      int cols, unsigned long long seed, int site, int block, unsigned thr, float scale_keep,
                                      void* stream) {
  DEVIT_CHECK(x && y && x_out && rows > 0 && cols > 0 && (!rowscale || rows_per_scale > 0), DEVIT_ERR_ARG,
              "devit_dropout_residual: bad argument");
  DEVIT_CHECK(cols % 4 == 0 && al16(x) && al16(y) && al16(x_out), DEVIT_ERR_ARG,
              "devit_dropout_residual: cols %d must be a multiple of 4 and the pointers 16-byte aligned", cols);
  const int rc = check_site("devit_dropout_residual", site, block, cols, cols);
  if (rc != DEVIT_OK) return rc;
  ResidualArgs a{x, y, x_out, rowscale, rows_per_scale, rows, cols, drop_key(seed, site, block, thr, scale_keep)};
  hipLaunchKernelGGL(dropout_residual_kernel, row_grid(rows, cols / 4), dim3(CX, RY), 0, (hipStream_t)stream, a);
  DEVIT_LAUNCH_CHECK();
  return DEVIT_OK;
}
