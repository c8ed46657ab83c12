// Deterministic mode: the switch, the workspace registry and the fold kernel (det.h); C entry points devit_set / get_deterministic,
// devit_det_workspace_bytes, devit_set_det_workspace.
#include <stdlib.h>

#include "det.h"

namespace {

int g_det = -1;     // -1: not set yet, take DEVIT_DETERMINISTIC from the environment

// one caller-owned workspace per device (a process that never asked for a device registers and finds device 0's)
constexpr int MAX_DEVICES = 16;
struct Ws {
  float* p;
  size_t bytes;
};
Ws g_ws[MAX_DEVICES];

int device_slot() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= MAX_DEVICES) dev = 0;
  return dev;
}

// One thread per output element, its S partials read in index order (the element's addresses are S slabs apart: every load of a wave is
// one contiguous row piece).  Memory-bound: S + 2 floats of traffic per element.
struct FoldArgs {
  const float* part;
  float* out;
  size_t slab;
  long long ldc, out_bs;
  int S, rows, cols, batch;
};
__global__ __launch_bounds__(256) void det_fold_kernel(const FoldArgs a) {
  const long long per_b = (long long)a.rows * a.cols, total = per_b * a.batch;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int b = (int)(i / per_b);
    const long long rc = i - (long long)b * per_b;
    const int r = (int)(rc / a.cols), c = (int)(rc - (long long)r * a.cols);
    const float* p = a.part + (size_t)b * a.S * a.slab + (size_t)r * a.cols + c;
    float f = p[0];
    for (int s = 1; s < a.S; ++s) f += p[(size_t)s * a.slab];
    float* o = a.out + (size_t)b * a.out_bs + (size_t)r * a.ldc + c;
    *o = *o + f;
  }
}

}  // namespace

bool devit_det::on() {
  if (g_det < 0) {
    const char* e = getenv("DEVIT_DETERMINISTIC");
    g_det = (e && atoi(e) == 1) ? 1 : 0;
  }
  return g_det == 1;
}

int devit_det::workspace(const char* who, size_t need_bytes, float** ws) {
  const Ws& w = g_ws[device_slot()];
  DEVIT_CHECK(w.p && w.bytes >= need_bytes, DEVIT_ERR_ARG,
              "%s: deterministic mode needs %zu bytes of workspace for this launch's partial sums, %zu are registered (devit_set_det_workspace; "
              "devit_det_workspace_bytes() covers the training step)", who, need_bytes, w.p ? w.bytes : (size_t)0);
  if (ws) *ws = w.p;
  return DEVIT_OK;
}

int devit_det::fold(const float* part, int S, size_t slab, int rows, int cols, float* out, long long ldc, int batch, long long out_bs,
                    hipStream_t s) {
  const FoldArgs a{part, out, slab, ldc, out_bs, S, rows, cols, batch};
  const long long total = (long long)rows * cols * batch;
  const long long blocks = (total + 255) / 256;
  hipLaunchKernelGGL(det_fold_kernel, dim3((unsigned)(blocks < 8192 ? blocks : 8192)), dim3(256), 0, s, a);
  DEVIT_LAUNCH_CHECK();
  return DEVIT_OK;
}

extern "C" int devit_set_deterministic(int on) {
  DEVIT_CHECK(on == 0 || on == 1, DEVIT_ERR_ARG, "devit_set_deterministic: %d is neither 0 nor 1", on);
  g_det = on;
  return DEVIT_OK;
}

extern "C" int devit_get_deterministic(void) { return devit_det::on() ? 1 : 0; }

// The largest launch of the training step: the grouped weight-gradient kernel at one 256 x 384 fp32 tile (+ 256 column sums) per (tile, slice) --
// one block's 19 tiles in 13 slices are 97 MB, a compacted student's 162 tiles in 3 slices 191 MB; the split-K 128 x 128 launches stay under
// 512 tiles of 64 KB (split_k_for).
extern "C" size_t devit_det_workspace_bytes(void) { return (size_t)256 << 20; }

extern "C" int devit_set_det_workspace(void* ws, size_t bytes) {
  DEVIT_CHECK((ws != nullptr) == (bytes > 0) && (((uintptr_t)ws) & 15) == 0, DEVIT_ERR_ARG,
              "devit_set_det_workspace: a 16-byte aligned device pointer with its size, or NULL and 0 to take it back");
  g_ws[device_slot()] = Ws{(float*)ws, bytes};
  return DEVIT_OK;
}
