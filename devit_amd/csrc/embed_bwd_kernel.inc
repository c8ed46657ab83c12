// The body of embed_bwd_kernel (elementwise.hip), included once per instantiation: EMBED_BWD_KERNEL names it; EMBED_BWD_DET == 0 is the default path's kernel
// (the batch slices' sums meet in dpos by fp32 atomics), 1 deterministic mode's: `dpos` is then the workspace, [slices][T * D], plain stores.
__global__ __launch_bounds__(256) void EMBED_BWD_KERNEL(const float* dx, int B, int T, int D, float* dpos,
                                                        __bf16* dx_bf16) {
  const int total = T * D / 4;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int d = (idx % (D / 4)) * 4, t = idx / (D / 4);
  const int b0 = (int)((long long)B * blockIdx.y / gridDim.y), b1 = (int)((long long)B * (blockIdx.y + 1) / gridDim.y);
  f32x4 s = {0.f, 0.f, 0.f, 0.f};
  auto one = [&](int b, f32x4& v) { v = load_stream((const f32x4*)(dx + ((size_t)b * T + t) * D + d)); };
  auto put = [&](int b, const f32x4& v) {
    s += v;
    if (dx_bf16) {
      const bf16x4 ob = {f2bf(v[0]), f2bf(v[1]), f2bf(v[2]), f2bf(v[3])};
      *(bf16x4*)(dx_bf16 + ((size_t)b * T + t) * D + d) = ob;
    }
  };
  int b = b0;
  for (; b + 4 <= b1; b += 4) {
    f32x4 v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) one(b + u, v[u]);
#pragma unroll
    for (int u = 0; u < 4; ++u) put(b + u, v[u]);
  }
  for (; b < b1; ++b) {
    f32x4 v;
    one(b, v);
    put(b, v);
  }
#if EMBED_BWD_DET
  *(f32x4*)(dpos + (size_t)blockIdx.y * T * D + (size_t)t * D + d) = s;
#else
  float* dst = dpos + (size_t)t * D + d;
#pragma unroll
  for (int e = 0; e < 4; ++e) unsafeAtomicAdd(dst + e, s[e]);
#endif
}
