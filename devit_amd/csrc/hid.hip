// Hidden-state distillation on the 16-bit path:
//   * the injection kernel of EncoderFn.backward: a gradient for an exposed 'encoder' output is added into the fp32 residual-stream
//     gradient between two block calls, and the bf16 branch gradient of the block below is rewritten from the sum (one rounding);
//   * cal_hid_relation_loss (utils/losses.py:295-304): row normalise, squared-difference statistics of the two Grams, the bf16 / fp32
//     S = coef (G_s - G_t) the gradient GEMM reads, and the backward of the row normalisation.  The Grams h h^T and dh^ = S h^ run on the
//     batched devit_gemm_bf16 (exact mode: devit_gemm_f32), as the q/k/v relation loss does.
#include "devit_common.h"
#include "reduce.h"

namespace {

inline unsigned grid_cap(size_t n, unsigned cap) {
  const size_t b = (n + 255) / 256;
  return (unsigned)(b < 1 ? 1 : (b > cap ? cap : b));
}

// dx += add (fp32, in place);  g = bf16((dx + add) * rowscale[row / rows_per_scale])
__global__ __launch_bounds__(256) void add_scale_cast_kernel(float* dx, const float* add, __bf16* g, const float* rowscale,
                                                             int rows_per_scale, int M, int D) {
  const size_t total = (size_t)M * D / 4;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int row = (int)(i * 4 / D);
    const float sc = rowscale ? rowscale[row / rows_per_scale] : 1.0f;
    const f32x4 v = *(const f32x4*)(dx + i * 4) + *(const f32x4*)(add + i * 4);
    *(f32x4*)(dx + i * 4) = v;
    const f32x4 s = v * sc;
    const bf16x4 o = {f2bf(s[0]), f2bf(s[1]), f2bf(s[2]), f2bf(s[3])};
    *(bf16x4*)(g + i * 4) = o;
  }
}

// ---- (a) row normalise: h^ = h / max(|h|, eps) into a packed [rows_total][ld] buffer (bf16, or fp32 in exact mode); columns >= D and rows >= M
//      are written as zeros (the Gram windows of the last images and the 128-wide GEMM tiles read them).  One wave per row, four columns
//      per lane and trip: D <= 1024 is four trips.
struct NormArgs {
  const float* h;
  void* out;
  float* inv;
  int M, D, ld, rows_total, out_f32;
  float eps;
};
__global__ __launch_bounds__(256) void hid_normalize_kernel(const NormArgs a) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= a.rows_total) return;
  f32x4 v[4];
  float ss = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int c = lane * 4 + k * 256;
    v[k] = (row < a.M && c < a.D) ? *(const f32x4*)(a.h + (size_t)row * a.D + c) : (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int e = 0; e < 4; ++e) ss += v[k][e] * v[k][e];
  }
  ss = wave_sum(ss);
  const float inv = 1.0f / fmaxf(sqrtf(ss), a.eps);
  if (row < a.M && lane == 0) a.inv[row] = inv;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int c = lane * 4 + k * 256;
    if (c >= a.ld) continue;
    const f32x4 o = v[k] * inv;       // (rows >= M and columns >= D hold zeros)
    if (a.out_f32) *(f32x4*)((float*)a.out + (size_t)row * a.ld + c) = o;
    else *(bf16x4*)((__bf16*)a.out + (size_t)row * a.ld + c) = (bf16x4){f2bf(o[0]), f2bf(o[1]), f2bf(o[2]), f2bf(o[3])};
  }
}

// ---- (b) statistics: row_sq[b][i] = sum_{j < N} (G_s[b][i][j] - G_t[b][i][j])^2 over the padded fp32 Grams [B][256][256]; one wave per row
__global__ __launch_bounds__(256) void hid_stats_kernel(const float* gs, const float* gt, int B, int N, float* row_sq) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= B * N) return;
  const int b = row / N, i = row % N;
  const size_t o = ((size_t)b * 256 + i) * 256 + lane * 4;
  const f32x4 vs = *(const f32x4*)(gs + o), vt = *(const f32x4*)(gt + o);
  float s = 0.f;
#pragma unroll
  for (int e = 0; e < 4; ++e)
    if (lane * 4 + e < N) {
      const float d = vs[e] - vt[e];
      s += d * d;
    }
  s = wave_sum(s);
  if (lane == 0) row_sq[row] = s;
}
// loss = scale * sum(row_sq): reduce.h's one block, fixed summation order (run-to-run deterministic)

// ---- (c) gradient: S = (coef * upstream) (G_s - G_t), bf16 (or fp32) [B][256][256], zero outside N x N; one wave per row
struct HidGradArgs {
  const float* gs; const float* gt;
  const float* upstream;   // device scalar (dL / dloss) or NULL (= 1)
  void* S;
  int N, out_f32;
  float coef;
};
__global__ __launch_bounds__(256) void hid_grad_kernel(const HidGradArgs a) {
  const int b = blockIdx.y, i = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int j0 = (threadIdx.x & 63) * 4;
  const size_t o = ((size_t)b * 256 + i) * 256 + j0;
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (i < a.N && j0 < a.N) {
    const float up = (a.upstream ? *a.upstream : 1.0f) * a.coef;
    const f32x4 vs = *(const f32x4*)(a.gs + o), vt = *(const f32x4*)(a.gt + o);
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (j0 + e < a.N) v[e] = (vs[e] - vt[e]) * up;
  }
  if (a.out_f32) *(f32x4*)((float*)a.S + o) = v;
  else *(bf16x4*)((__bf16*)a.S + o) = (bf16x4){f2bf(v[0]), f2bf(v[1]), f2bf(v[2]), f2bf(v[3])};
}

// ---- (d) normalise backward: dh = inv (dh^ - h^ (h^ . dh^)), fp32 [M][D]; h^ is the forward's packed buffer (bf16 or fp32, leading dimension ld),
//      dh^ fp32 with the same leading dimension.  One wave per row; nothing is written past row M - 1 or column D - 1.
struct NormBwdArgs {
  const void* hn;
  const float* dhn;
  const float* inv;
  float* dh;
  int M, D, ld, hn_f32;
};
__global__ __launch_bounds__(256) void hid_normalize_bwd_kernel(const NormBwdArgs a) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= a.M) return;
  f32x4 hv[4], dv[4];
  float p = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int c = lane * 4 + k * 256;
    hv[k] = dv[k] = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (c < a.D) {
      if (a.hn_f32) hv[k] = *(const f32x4*)((const float*)a.hn + (size_t)row * a.ld + c);
      else {
        const bf16x4 t = *(const bf16x4*)((const __bf16*)a.hn + (size_t)row * a.ld + c);
        hv[k] = (f32x4){bf2f(t[0]), bf2f(t[1]), bf2f(t[2]), bf2f(t[3])};
      }
      dv[k] = *(const f32x4*)(a.dhn + (size_t)row * a.ld + c);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) p += hv[k][e] * dv[k][e];
  }
  p = wave_sum(p);
  const float inv = a.inv[row];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int c = lane * 4 + k * 256;
    if (c < a.D) *(f32x4*)(a.dh + (size_t)row * a.D + c) = (dv[k] - hv[k] * p) * inv;
  }
}

inline bool aligned16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

int check_hid_dims(const char* who, int B, int N, int D, int ld) {
  DEVIT_CHECK(B > 0 && N > 0 && N <= 208 && D > 0 && D <= 1024 && D % 64 == 0 && ld >= D && ld <= 1024 && ld % 128 == 0 &&
                  (long long)B * N < (1ll << 31) - 256,
              DEVIT_ERR_SHAPE, "%s: B=%d N=%d D=%d ld=%d: N <= 208, D a multiple of 64 up to 1024, ld a multiple of 128 from D to 1024", who, B,
              N, D, ld);
  return DEVIT_OK;
}

}  // namespace

extern "C" int devit_add_scale_cast_bf16(float* dx, const float* add, void* g_bf16, const float* rowscale, int rows_per_scale, int M,
                                         int D, void* stream) {
  DEVIT_CHECK(dx && add && g_bf16 && (!rowscale || rows_per_scale > 0), DEVIT_ERR_ARG, "devit_add_scale_cast_bf16: bad argument");
  DEVIT_CHECK(aligned16(dx) && aligned16(add) && (((uintptr_t)g_bf16) & 7) == 0, DEVIT_ERR_ARG, "devit_add_scale_cast_bf16: alignment");
  DEVIT_CHECK(D > 0 && D % 4 == 0 && M > 0, DEVIT_ERR_SHAPE, "devit_add_scale_cast_bf16: M=%d, D=%d must be positive, D a multiple of 4", M, D);
  hipLaunchKernelGGL(add_scale_cast_kernel, dim3(grid_cap((size_t)M * D / 4, 4096)), dim3(256), 0, (hipStream_t)stream, dx, add,
                     (__bf16*)g_bf16, rowscale, rows_per_scale, M, D);
  DEVIT_LAUNCH_CHECK();
  return DEVIT_OK;
}

extern "C" int devit_hid_normalize(const float* h, void* out, float* inv, int B, int N, int D, int ld, int rows_total, int out_is_f32,
                                   float eps, void* stream) {
  DEVIT_CHECK(h && out && inv && aligned16(h) && aligned16(out) && eps > 0.f, DEVIT_ERR_ARG, "devit_hid_normalize: bad argument");
  int rc = check_hid_dims("devit_hid_normalize", B, N, D, ld);
  if (rc != DEVIT_OK) return rc;
  DEVIT_CHECK(rows_total >= B * N, DEVIT_ERR_SHAPE, "devit_hid_normalize: rows_total=%d < B * N = %d", rows_total, B * N);
  NormArgs a{h, out, inv, B * N, D, ld, rows_total, out_is_f32 != 0, eps};
  hipLaunchKernelGGL(hid_normalize_kernel, dim3((rows_total + 3) / 4), dim3(256), 0, (hipStream_t)stream, a);
  DEVIT_LAUNCH_CHECK();
  return DEVIT_OK;
}

extern "C" int devit_hid_stats(const float* gram_s, const float* gram_t, int B, int N, int ldr, int layers, float* row_sq, float* loss,
                               void* stream) {
  DEVIT_CHECK(gram_s && gram_t && row_sq && loss && aligned16(gram_s) && aligned16(gram_t), DEVIT_ERR_ARG, "devit_hid_stats: bad argument");
  DEVIT_CHECK(B > 0 && N > 0 && N <= 208 && ldr == 256 && layers > 0 && (long long)B * N < (1ll << 31) - 256, DEVIT_ERR_SHAPE,
              "devit_hid_stats: B=%d N=%d ldr=%d layers=%d: N <= 208, padded Grams 256 wide", B, N, ldr, layers);
  hipLaunchKernelGGL(hid_stats_kernel, dim3((B * N + 3) / 4), dim3(256), 0, (hipStream_t)stream, gram_s, gram_t, B, N, row_sq);
  DEVIT_LAUNCH_CHECK();
  const float scale = (float)(1.0 / ((double)B * N * N * layers));
  hipLaunchKernelGGL(fixed_order_reduce_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, (const float*)row_sq, (long long)B * N, scale, loss);
  DEVIT_LAUNCH_CHECK();
  return DEVIT_OK;
}

extern "C" int devit_hid_grad(const float* gram_s, const float* gram_t, const float* upstream, int B, int N, int ldr, int layers, void* S_out,
                              int out_is_f32, void* stream) {
  DEVIT_CHECK(gram_s && gram_t && S_out && aligned16(gram_s) && aligned16(gram_t) && aligned16(S_out), DEVIT_ERR_ARG,
              "devit_hid_grad: bad argument");
  DEVIT_CHECK(B > 0 && B <= 65535 && N > 0 && N <= 208 && ldr == 256 && layers > 0, DEVIT_ERR_SHAPE,
              "devit_hid_grad: B=%d N=%d ldr=%d layers=%d: B <= 65535, N <= 208, padded Grams 256 wide", B, N, ldr, layers);
  HidGradArgs a{gram_s, gram_t, upstream, S_out, N, out_is_f32 != 0, (float)(4.0 / ((double)B * N * N * layers))};
  hipLaunchKernelGGL(hid_grad_kernel, dim3(64, B), dim3(256), 0, (hipStream_t)stream, a);
  DEVIT_LAUNCH_CHECK();
  return DEVIT_OK;
}

extern "C" int devit_hid_normalize_bwd(const void* hn, const float* dhn, const float* inv, float* dh, int B, int N, int D, int ld,
                                       int hn_is_f32, void* stream) {
  DEVIT_CHECK(hn && dhn && inv && dh && aligned16(hn) && aligned16(dhn) && aligned16(dh), DEVIT_ERR_ARG, "devit_hid_normalize_bwd: bad argument");
  int rc = check_hid_dims("devit_hid_normalize_bwd", B, N, D, ld);
  if (rc != DEVIT_OK) return rc;
  NormBwdArgs a{hn, dhn, inv, dh, B * N, D, ld, hn_is_f32 != 0};
  hipLaunchKernelGGL(hid_normalize_bwd_kernel, dim3((B * N + 3) / 4), dim3(256), 0, (hipStream_t)stream, a);
  DEVIT_LAUNCH_CHECK();
  return DEVIT_OK;
}
