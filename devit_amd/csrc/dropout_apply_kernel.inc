// The body of dropout_apply_kernel (dropout.hip), included once per instantiation: DROPOUT_APPLY_KERNEL names it; DROPOUT_APPLY_DET == 0 is the default
// path's kernel (the row strips' column sums meet in colsum by fp32 atomics), 1 deterministic mode's: `colsum` is then the workspace, [strips][cols].
template <bool F32>
__global__ __launch_bounds__(CX* RY) void DROPOUT_APPLY_KERNEL(const ApplyArgs a) {
  constexpr int V = F32 ? 4 : 8;
  __shared__ float red[RY][CX][V];
  const int c0 = (blockIdx.x * CX + threadIdx.x) * V;
  const bool live = c0 < a.cols;
  float acc[V];
#pragma unroll
  for (int e = 0; e < V; ++e) acc[e] = 0.f;
  if (live) {
    for (int r = blockIdx.y * RY + threadIdx.y; r < a.rows; r += gridDim.y * RY) {
      const unsigned long long e0 = (unsigned long long)r * (unsigned long long)a.pitch + (unsigned long long)c0;
      if constexpr (F32) {
        float* p = (float*)a.x + (size_t)r * a.ld + c0;
        f32x4 v = *(const f32x4*)p;
        const u32x4 w = drop_words(a.d, e0);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          v[e] = w[e] >= a.d.thr ? v[e] * a.d.s : 0.f;
          acc[e] += v[e];
        }
        *(f32x4*)p = v;
      } else {
        __bf16* p = (__bf16*)a.x + (size_t)r * a.ld + c0;
        bf16x8 v = *(const bf16x8*)p;
        const u32x4 w0 = drop_words(a.d, e0), w1 = drop_words(a.d, e0 + 4);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const unsigned w = e < 4 ? w0[e] : w1[e - 4];
          v[e] = f2bf(w >= a.d.thr ? bf2f(v[e]) * a.d.s : 0.f);
          acc[e] += bf2f(v[e]);          // the sums are of what the buffer now holds (a Linear's bias gradient when it is a dY)
        }
        *(bf16x8*)p = v;
      }
    }
  }
  if (a.colsum) {                        // (uniform over the grid)
#pragma unroll
    for (int e = 0; e < V; ++e) red[threadIdx.y][threadIdx.x][e] = acc[e];
    __syncthreads();
    if (threadIdx.y == 0 && live) {
#pragma unroll
      for (int e = 0; e < V; ++e) {
        float s = red[0][threadIdx.x][e];
#pragma unroll
        for (int y = 1; y < RY; ++y) s += red[y][threadIdx.x][e];
#if DROPOUT_APPLY_DET
        a.colsum[(size_t)blockIdx.y * a.cols + c0 + e] = s;
#else
        atomicAdd(a.colsum + c0 + e, s);
#endif
      }
    }
  }
}
