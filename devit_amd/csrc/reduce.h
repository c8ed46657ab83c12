// The fixed-order reduce behind the row-wise loss kernels (losses.hip, relation.hip, qkvce.hip, hid.hip): out[blockIdx.x] = scale * sum of segment
// blockIdx.x of src, segments of n floats.  One block of 1024 threads per segment, 8 independent partial sums per thread (50688 values: six
// 16-byte-strided trips instead of 198 dependent ones), a tree over the eight, the wave's shuffles, then the 16 wave partials in order: no atomics,
// so the result is run-to-run deterministic.  Launch: dim3(segments), dim3(1024).
#pragma once
#include "devit_common.h"

namespace {

__global__ __launch_bounds__(1024) void fixed_order_reduce_kernel(const float* src, long long n, float scale, float* out) {
  __shared__ float red[16];
  src += (size_t)blockIdx.x * n;
  float p[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (long long i0 = threadIdx.x; i0 < n; i0 += 8 * 1024) {
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const long long i = i0 + u * 1024;
      p[u] += i < n ? src[i] : 0.f;
    }
  }
  float s = ((p[0] + p[1]) + (p[2] + p[3])) + ((p[4] + p[5]) + (p[6] + p[7]));
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = 0.f;
#pragma unroll
    for (int w = 0; w < 16; ++w) t += red[w];
    out[blockIdx.x] = t * scale;
  }
}

}  // namespace
