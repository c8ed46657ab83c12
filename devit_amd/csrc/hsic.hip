// Unit ranking of the shrink stage (devit_amd/shrink.py: neuron_scores / head_scores; core/imp_rank.py:16-47, :93-129, :175-239):
// the HSIC relevance of every MLP neuron / attention head against the softmax of the logits, the neurons' activation mass and the heads'
// mutual redundancy, without a [units, B, B] tensor in HBM for the neurons and without a vendor BLAS.
//
//   feature of sample a for unit u: x_a[n] = mean of `group` consecutive channels of X[a, n, u * group ...], n < N tokens
//   Kmix_u[a, b] = 1/5 sum_{s in 1,2,4,8,16} exp(-d2(a, b) / (2 s^2)),   d2(a, b) = sum_n (x_a[n] - x_b[n])^2
//   rel[u] = sum_ab Kmix_u[a, b] W[a, b]         W = center(y y^T), y = softmax(logits) - column mean    (devit_hsic_target)
//          = sum_ab (Kmix_u - 1)[a, b] W[a, b]   (W is centred: a constant does not enter; gauss_mix_m1 says why that form is computed)
//   act[u] = sum_{a, n} |X[a, n, u]|             (group == 1)
//   red[h] = 1/(H - 1) sum_{g != h} sum_ab Kmix_h[a, b] center(Kmix_g)[a, b]                               (devit_hsic_head_pairs)
//
// trace(center(A) center(B)) = sum A o center(B): only the target side is centred.  The reference's `mean_sub` shifts every sample of a
// feature column by the same constant mean / (std + 1e-12), which pairwise distances cannot see: d2 is taken from the raw values as a sum of
// squared DIFFERENCES in fp32 (the Gram form nrm_a + nrm_b - 2 <a, b> cancels once that constant is large).  A column that is constant and
// non-zero over the batch has std = 0 and the reference's shift is mean * 1e12 -- its result is cancellation noise; the value here is the
// translation-invariant one.
//
// Two steps per call of devit_hsic_scores: hsic_pack_kernel turns the strided 16-bit / fp32 rows [B][N][units * group] into unit-major fp32
// slices ws[u][n][Bp] (Bp = B rounded up to 64, zero padded; the group mean is taken here), so that everything the pair kernel reads is
// contiguous; hsic_pair_kernel gives one workgroup a unit, walks the 64 x 64 tiles of the upper triangle of (a, b) with a 4 x 4 block of
// pairs per thread, 33 tokens at a time through LDS, applies the five exponentials (as exp - 1) to the finished d2 and reduces against W in registers
// (double accumulators for the two reductions: the sum against W cancels).  One workgroup owns a unit's whole sum: no atomics, the
// result does not depend on the launch's timing.
#include "devit_common.h"

namespace {

constexpr int HSIC_MAX_B = 256, HSIC_MAX_HEADS = 16, HSIC_TILE = 64, HSIC_NC = 33;

template <typename T>
__device__ __forceinline__ float hsic_ld(const T* p) {
  return (float)*p;
}

__device__ __forceinline__ double block_sum_double(double v, double* red /* [4] LDS */) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}

// ---- target: W = center(y y^T) = z z^T with z = y centred twice over the batch (H G H = (H y)(H y)^T) ----------------------------------
__global__ __launch_bounds__(256) void hsic_softmax_kernel(const float* y, float* z, int C, int softmax) {
  const float* row = y + (size_t)blockIdx.x * C;
  float* out = z + (size_t)blockIdx.x * C;
  if (!softmax) {
    for (int c = threadIdx.x; c < C; c += 256) out[c] = row[c];
    return;
  }
  __shared__ float redm[4];
  __shared__ double reds[4];
  float m = -INFINITY;
  for (int c = threadIdx.x; c < C; c += 256) m = fmaxf(m, row[c]);
  m = wave_max(m);
  if ((threadIdx.x & 63) == 0) redm[threadIdx.x >> 6] = m;
  __syncthreads();
  m = fmaxf(fmaxf(redm[0], redm[1]), fmaxf(redm[2], redm[3]));
  double s = 0.0;
  for (int c = threadIdx.x; c < C; c += 256) s += (double)expf(row[c] - m);
  s = block_sum_double(s, reds);
  const float inv = (float)(1.0 / s);
  for (int c = threadIdx.x; c < C; c += 256) out[c] = expf(row[c] - m) * inv;
}

__global__ __launch_bounds__(256) void hsic_center_columns_kernel(float* z, int B, int C) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  for (int pass = 0; pass < 2; ++pass) {
    double s = 0.0;
    for (int a = 0; a < B; ++a) s += (double)z[(size_t)a * C + c];
    const float mean = (float)(s / B);
    for (int a = 0; a < B; ++a) z[(size_t)a * C + c] -= mean;
  }
}

__global__ __launch_bounds__(256) void hsic_gram_kernel(const float* z, float* W, int B, int C) {
  __shared__ float za[256];
  const int a = blockIdx.x, b = threadIdx.x;
  double acc = 0.0;
  for (int c0 = 0; c0 < C; c0 += 256) {
    __syncthreads();
    if (c0 + threadIdx.x < C) za[threadIdx.x] = z[(size_t)a * C + c0 + threadIdx.x];
    __syncthreads();
    if (b < B) {
      const int cnt = min(256, C - c0);
      const float* zb = z + (size_t)b * C + c0;
      for (int c = 0; c < cnt; ++c) acc += (double)za[c] * (double)zb[c];
    }
  }
  if (b < B) W[(size_t)a * B + b] = (float)acc;
}

// ---- pack: X[a][n][u * group + g] (strided, any of three element types) -> ws[u][n][Bp] fp32 ---------------------------------------------
// group == 1: 64 samples x 64 channels of one token through LDS (reads whole lines of the channel rows, writes whole lines of the slices)
template <typename T>
__global__ __launch_bounds__(256) void hsic_pack_kernel(const T* X, long long sb, long long sn, int B, int Bp, int N, int units, float* ws) {
  __shared__ float tile[64][65];
  const int c0 = blockIdx.x * 64, n = blockIdx.y, a0 = blockIdx.z * 64;
  const int lane = threadIdx.x & 63, q = threadIdx.x >> 6;
#pragma unroll 4
  for (int i = 0; i < 16; ++i) {
    const int a = a0 + q + 4 * i, c = c0 + lane;
    tile[lane][q + 4 * i] = (a < B && c < units) ? hsic_ld(X + (long long)a * sb + (long long)n * sn + c) : 0.f;
  }
  __syncthreads();
#pragma unroll 4
  for (int i = 0; i < 16; ++i) {
    const int c = c0 + q + 4 * i;
    if (c < units) ws[((size_t)c * N + n) * Bp + a0 + lane] = tile[q + 4 * i][lane];
  }
}

// group > 1 (heads: a few units, little data): one thread per (sample, token, unit), the unit fastest
template <typename T>
__global__ __launch_bounds__(256) void hsic_pack_group_kernel(const T* X, long long sb, long long sn, int B, int Bp, int N, int units, int group,
                                                              float* ws) {
  const long long total = (long long)Bp * N * units;
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int u = (int)(e % units), n = (int)((e / units) % N), a = (int)(e / ((long long)units * N));
  float s = 0.f;
  if (a < B) {
    const T* p = X + (long long)a * sb + (long long)n * sn + (long long)u * group;
    for (int g = 0; g < group; ++g) s += hsic_ld(p + g);
    s /= (float)group;
  }
  ws[((size_t)u * N + n) * Bp + a] = s;
}

// ---- pairs ---------------------------------------------------------------------------------------------------------------------------
// exp(t) - 1 for t <= 0 without the cancellation at small |t|: degree-7 Taylor below 1/4 (remainder 4e-10), v_exp_f32 above
__device__ __forceinline__ float expm1_neg(float t) {
  const float p = t * fmaf(t, fmaf(t, fmaf(t, fmaf(t, fmaf(t, fmaf(t, 1.f / 5040.f, 1.f / 720.f), 1.f / 120.f), 1.f / 24.f), 1.f / 6.f), 0.5f), 1.f);
  const float e = __builtin_amdgcn_exp2f(t * LOG2E) - 1.f;
  return t > -0.25f ? p : e;
}
// Kmix - 1 = 1/5 sum_s (exp(-d2 / (2 s^2)) - 1), s = 1, 2, 4, 8, 16.  Both sums this feeds are against CENTRED kernels (W, center(Kmix_g)), which a
// constant does not enter; on a real model the samples of a head lie close together, Kmix is within 1e-3 of 1 and an fp32 Kmix would round away
// the part that carries the signal (emulated on the CPU: 3e-4 of the largest score at a spread of 1 % of the feature, against 5e-8 in this form).
__device__ __forceinline__ float gauss_mix_m1(float d2) {
  const float e = expm1_neg(d2 * -0.5f) + expm1_neg(d2 * -0.125f) + expm1_neg(d2 * -0.03125f) + expm1_neg(d2 * -0.0078125f) +
                  expm1_neg(d2 * -0.001953125f);
  return e * 0.2f;
}

__global__ __launch_bounds__(256) void hsic_pair_kernel(const float* ws, const float* W, int B, int Bp, int N, float* rel, float* act,
                                                        float* kmix1) {
  __shared__ __attribute__((aligned(16))) float xa[HSIC_NC][HSIC_TILE];
  __shared__ __attribute__((aligned(16))) float xb[HSIC_NC][HSIC_TILE];
  __shared__ double red[4];
  const int u = blockIdx.x, tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
  const float* xu = ws + (size_t)u * N * Bp;
  float* ku = kmix1 ? kmix1 + (size_t)u * B * B : nullptr;
  const int nt = Bp / HSIC_TILE;
  double relacc = 0.0, actacc = 0.0;
  for (int ta = 0; ta < nt; ++ta) {
    for (int tb = ta; tb < nt; ++tb) {
      float d[4][4];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) d[i][j] = 0.f;
      for (int n0 = 0; n0 < N; n0 += HSIC_NC) {
        const int cnt = min(HSIC_NC, N - n0);
        __syncthreads();
        for (int idx = tid; idx < cnt * 16; idx += 256) {
          const int r = idx >> 4, c4 = (idx & 15) * 4;
          const float* src = xu + (size_t)(n0 + r) * Bp + c4;
          const f32x4 va = *(const f32x4*)(src + ta * HSIC_TILE);
          const f32x4 vb = *(const f32x4*)(src + tb * HSIC_TILE);
          *(f32x4*)&xa[r][c4] = va;
          *(f32x4*)&xb[r][c4] = vb;
          if (ta == tb) actacc += (double)(fabsf(va[0]) + fabsf(va[1])) + (double)(fabsf(va[2]) + fabsf(va[3]));
        }
        __syncthreads();
        for (int r = 0; r < cnt; ++r) {
          const f32x4 a4 = *(const f32x4*)&xa[r][ty * 4];
          const f32x4 b4 = *(const f32x4*)&xb[r][tx * 4];
#pragma unroll
          for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const float t = a4[i] - b4[j];
              d[i][j] = fmaf(t, t, d[i][j]);
            }
        }
      }
      const double weight = ta == tb ? 1.0 : 2.0;       // Kmix and W are symmetric: the lower triangle's tiles are not walked
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int a = ta * HSIC_TILE + ty * 4 + i;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int b = tb * HSIC_TILE + tx * 4 + j;
          if (a < B && b < B) {
            const float k = gauss_mix_m1(d[i][j]);
            relacc += weight * (double)k * (double)W[(size_t)a * B + b];
            if (ku) {
              ku[(size_t)a * B + b] = k;
              if (ta != tb) ku[(size_t)b * B + a] = k;
            }
          }
        }
      }
    }
  }
  relacc = block_sum_double(relacc, red);
  if (tid == 0) rel[u] = (float)relacc;
  if (act) {
    actacc = block_sum_double(actacc, red);
    if (tid == 0) act[u] = (float)actacc;
  }
}

// ---- heads: red[h] = 1/(H-1) sum_{g != h} <Kmix_h, center(Kmix_g)> = the same with Kmix - 1 on both sides (kmix1) ------------------------------------------------------------------------
__global__ __launch_bounds__(256) void hsic_head_pairs_kernel(const float* kmix, int H, int B, float* out) {
  __shared__ double rowmean[HSIC_MAX_HEADS][HSIC_MAX_B];
  __shared__ double total[HSIC_MAX_HEADS];
  __shared__ double red[4];
  const int h = blockIdx.x, tid = threadIdx.x;
  for (int g = 0; g < H; ++g) {
    double s = 0.0;
    if (tid < B) {
      const float* row = kmix + ((size_t)g * B + tid) * B;
      for (int b = 0; b < B; ++b) s += (double)row[b];
      rowmean[g][tid] = s / B;
    }
    s = block_sum_double(s, red);
    if (tid == 0) total[g] = s / ((double)B * B);
  }
  __syncthreads();
  const float* kh = kmix + (size_t)h * B * B;
  double acc = 0.0;
  for (int e = tid; e < B * B; e += 256) {
    const int a = e / B, b = e - a * B;
    double c = 0.0;
    for (int g = 0; g < H; ++g)
      if (g != h) c += (double)kmix[(size_t)g * B * B + e] - rowmean[g][a] - rowmean[g][b] + total[g];     // Kmix is symmetric: column mean = row mean
    acc += (double)kh[e] * c;
  }
  acc = block_sum_double(acc, red);
  if (tid == 0) out[h] = (float)(acc / (H - 1));
}

template <typename T>
void launch_pack(const void* X, long long sb, long long sn, int B, int Bp, int N, int units, int group, float* ws, hipStream_t st) {
  if (group == 1) {
    hipLaunchKernelGGL(hsic_pack_kernel<T>, dim3((units + 63) / 64, N, Bp / 64), dim3(256), 0, st, (const T*)X, sb, sn, B, Bp, N, units, ws);
  } else {
    const long long total = (long long)Bp * N * units;
    hipLaunchKernelGGL(hsic_pack_group_kernel<T>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, (const T*)X, sb, sn, B, Bp, N, units,
                       group, ws);
  }
}

bool aligned16(const void* p) { return ((size_t)p & 15) == 0; }

}  // namespace

extern "C" int devit_hsic_target(const float* y, int B, int C, int softmax, float* W, void* workspace, size_t workspace_bytes, void* stream) {
  DEVIT_CHECK(y && W && workspace, DEVIT_ERR_ARG, "devit_hsic_target: null pointer");
  DEVIT_CHECK(B >= 2 && B <= HSIC_MAX_B && C >= 1 && C <= (1 << 20), DEVIT_ERR_ARG, "devit_hsic_target: B = %d (2..%d), C = %d unsupported", B,
              HSIC_MAX_B, C);
  DEVIT_CHECK(workspace_bytes >= (size_t)B * C * sizeof(float), DEVIT_ERR_ARG, "devit_hsic_target: workspace %zu B < B * C * 4 = %zu B",
              workspace_bytes, (size_t)B * C * sizeof(float));
  hipStream_t st = (hipStream_t)stream;
  float* z = (float*)workspace;
  hipLaunchKernelGGL(hsic_softmax_kernel, dim3(B), dim3(256), 0, st, y, z, C, softmax);
  hipLaunchKernelGGL(hsic_center_columns_kernel, dim3((C + 255) / 256), dim3(256), 0, st, z, B, C);
  hipLaunchKernelGGL(hsic_gram_kernel, dim3(B), dim3(256), 0, st, (const float*)z, W, B, C);
  DEVIT_LAUNCH_CHECK();
  return DEVIT_OK;
}

extern "C" size_t devit_hsic_scores_workspace(int B, int N, int units) {
  if (B < 2 || B > HSIC_MAX_B || N < 1 || units < 1) return 0;
  return (size_t)units * N * ((B + HSIC_TILE - 1) / HSIC_TILE * HSIC_TILE) * sizeof(float);
}

extern "C" int devit_hsic_scores(const void* X, int elem, int B, int N, int units, int group, long long batch_stride, long long token_stride,
                                 const float* W, float* rel, float* act, float* kmix1, void* workspace, size_t workspace_bytes, void* stream) {
  DEVIT_CHECK(X && W && rel && workspace, DEVIT_ERR_ARG, "devit_hsic_scores: null pointer");
  DEVIT_CHECK(elem == DEVIT_HSIC_BF16 || elem == DEVIT_HSIC_F16 || elem == DEVIT_HSIC_F32, DEVIT_ERR_ARG, "devit_hsic_scores: element type %d",
              elem);
  DEVIT_CHECK(B >= 2 && B <= HSIC_MAX_B, DEVIT_ERR_ARG, "devit_hsic_scores: B = %d outside 2..%d (rank on a smaller batch, or on several: rank_units(batches=))",
              B, HSIC_MAX_B);
  DEVIT_CHECK(N >= 1 && N <= 65535 && units >= 1 && units <= (1 << 20) && group >= 1 && group <= 4096, DEVIT_ERR_ARG,
              "devit_hsic_scores: N = %d, units = %d, group = %d unsupported", N, units, group);
  DEVIT_CHECK(token_stride >= (long long)units * group && batch_stride >= (long long)(N - 1) * token_stride + (long long)units * group,
              DEVIT_ERR_ARG, "devit_hsic_scores: strides (batch %lld, token %lld) overlap for N = %d, units * group = %d", batch_stride,
              token_stride, N, units * group);
  DEVIT_CHECK(!(act && group != 1), DEVIT_ERR_ARG, "devit_hsic_scores: act is defined for group == 1 (neurons) only");
  const size_t need = devit_hsic_scores_workspace(B, N, units);
  DEVIT_CHECK(workspace_bytes >= need && aligned16(workspace), DEVIT_ERR_ARG, "devit_hsic_scores: workspace %zu B < %zu B, or not 16-byte aligned",
              workspace_bytes, need);
  hipStream_t st = (hipStream_t)stream;
  const int Bp = (B + HSIC_TILE - 1) / HSIC_TILE * HSIC_TILE;
  float* ws = (float*)workspace;
  if (elem == DEVIT_HSIC_BF16)
    launch_pack<__bf16>(X, batch_stride, token_stride, B, Bp, N, units, group, ws, st);
  else if (elem == DEVIT_HSIC_F16)
    launch_pack<_Float16>(X, batch_stride, token_stride, B, Bp, N, units, group, ws, st);
  else
    launch_pack<float>(X, batch_stride, token_stride, B, Bp, N, units, group, ws, st);
  hipLaunchKernelGGL(hsic_pair_kernel, dim3(units), dim3(256), 0, st, (const float*)ws, W, B, Bp, N, rel, act, kmix1);
  DEVIT_LAUNCH_CHECK();
  return DEVIT_OK;
}

extern "C" int devit_hsic_head_pairs(const float* kmix1, int H, int B, float* red, void* stream) {
  DEVIT_CHECK(kmix1 && red, DEVIT_ERR_ARG, "devit_hsic_head_pairs: null pointer");
  DEVIT_CHECK(H >= 2 && H <= HSIC_MAX_HEADS && B >= 2 && B <= HSIC_MAX_B, DEVIT_ERR_ARG, "devit_hsic_head_pairs: H = %d (2..%d), B = %d (2..%d)", H,
              HSIC_MAX_HEADS, B, HSIC_MAX_B);
  hipLaunchKernelGGL(hsic_head_pairs_kernel, dim3(H), dim3(256), 0, (hipStream_t)stream, kmix1, H, B, red);
  DEVIT_LAUNCH_CHECK();
  return DEVIT_OK;
}
