// DEKD loss kernels: fused logit-distillation loss (+ its gradient) and the row-softmax / KL part of
// the q/k/v feature-relation loss (the Gram products run on the MFMA GEMM, see relation_* in ops.py).
//   cls loss   : utils/losses.py:135-177 (DistillLoss) + timm SoftTargetCrossEntropy
//   relation   : utils/losses.py:307-328 (feature_relation_loss), closed form in SURVEY.md App. A
#include "det.h"
#include "devit_common.h"
#include "reduce.h"

namespace {

constexpr int MAXC_PER_LANE = 16;  // classes <= 1024

struct ClsArgs {
  const float* lo;      // student cls-head logits [B][C]
  const float* lk;      // student dist-head logits [B][C]
  const float* lt;      // teacher logits [B][C]
  const float* y;       // soft targets [B][C]
  float* loss;          // [3]: total, base, distill
  float* dlo;           // [B][C] d total / d lo
  float* dlk;
  int B, C, kind;       // kind: 0 none, 1 soft, 2 hard
  float alpha, tau;
};

__device__ __forceinline__ void row_lse(const float (&x)[MAXC_PER_LANE], int n, float inv_t, float& mx, float& lse) {
  mx = -INFINITY;
#pragma unroll
  for (int i = 0; i < MAXC_PER_LANE; ++i)
    if (i < n) mx = fmaxf(mx, x[i] * inv_t);
  mx = wave_max(mx);
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < MAXC_PER_LANE; ++i)
    if (i < n) s += expf(x[i] * inv_t - mx);
  s = wave_sum(s);
  lse = mx + logf(s);
}

// One wave per row, 16 rows per workgroup, B / 16 workgroups; each workgroup adds its weighted share to the three loss
// scalars (zeroed by the launcher) with fp32 atomics -- 16 adds per scalar at B = 256.  (One workgroup walking all rows
// was a 135 us chain of dependent row reductions.)
#define CLS_LOSS_KERNEL cls_loss_kernel
#define CLS_LOSS_DET 0
#include "cls_loss_kernel.inc"
#undef CLS_LOSS_KERNEL
#undef CLS_LOSS_DET
#define CLS_LOSS_KERNEL cls_loss_det_kernel
#define CLS_LOSS_DET 1
#include "cls_loss_kernel.inc"
#undef CLS_LOSS_KERNEL
#undef CLS_LOSS_DET

// ---- relation loss, stage 1: per-row log-sum-exp of R/sqrt(hd) for teacher and student Grams, and the
//      row's KL contribution sum_j e^{t_ij}(t_ij - s_ij).  R_* are [B][ldr][ldr] f32 (padded Grams).
struct RelStatArgs {
  const float* rt; const float* rs;
  float* lse_t; float* lse_s;   // [B][N]
  float* row_kl;                // [B][N]
  int B, N, ldr;
  float inv_sqrt_t, inv_sqrt_s;
};
__global__ __launch_bounds__(256) void rel_stats_kernel(const RelStatArgs a) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= a.B * a.N) return;
  const int b = row / a.N, i = row % a.N;
  // one 16-byte load per lane and matrix: columns 4 lane .. 4 lane + 3 of the 256-wide padded Gram row
  const f32x4 vt = lane * 4 < a.ldr ? *(const f32x4*)(a.rt + ((size_t)b * a.ldr + i) * a.ldr + lane * 4) : (f32x4){0.f, 0.f, 0.f, 0.f};
  const f32x4 vs = lane * 4 < a.ldr ? *(const f32x4*)(a.rs + ((size_t)b * a.ldr + i) * a.ldr + lane * 4) : (f32x4){0.f, 0.f, 0.f, 0.f};
  float t[4], s[4];
  float mt = -INFINITY, ms = -INFINITY;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int j = lane * 4 + k;
    t[k] = j < a.N ? vt[k] * a.inv_sqrt_t : -INFINITY;
    s[k] = j < a.N ? vs[k] * a.inv_sqrt_s : -INFINITY;
    mt = fmaxf(mt, t[k]);
    ms = fmaxf(ms, s[k]);
  }
  mt = wave_max(mt);
  ms = wave_max(ms);
  float st = 0.f, ss = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    st += expf(t[k] - mt);
    ss += expf(s[k] - ms);
  }
  const float lt = mt + logf(wave_sum(st)), ls = ms + logf(wave_sum(ss));
  float kl = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (lane * 4 + k < a.N) {
      const float a_t = t[k] - lt, a_s = s[k] - ls;
      kl += expf(a_t) * (a_t - a_s);
    }
  kl = wave_sum(kl);
  if (lane == 0) {
    a.lse_t[row] = lt;
    a.lse_s[row] = ls;
    a.row_kl[row] = kl;
  }
}
// loss = sum(row_kl) / B   (KLDivLoss batchmean, utils/losses.py:309): reduce.h's one block, fixed summation order
// stage 2 (backward): S = G + G^T with G = (softmax(R_s) - softmax(R_t)) * upstream / (B sqrt(hd_s)); the Gram
// is symmetric, so S_ij = e^{rs_ij}(e^{-ls_i} + e^{-ls_j}) - e^{rt_ij}(e^{-lt_i} + e^{-lt_j}).  bf16 [B][ldr][ldr],
// zero outside N x N; dF_student = S F_student runs on the MFMA GEMM.
struct RelGradArgs {
  const float* rt; const float* rs; const float* lse_t; const float* lse_s;
  const float* upstream;  // device scalar (dL/dloss) or NULL (= 1)
  void* S;
  int B, N, ldr, out_f32;
  float inv_sqrt_t, inv_sqrt_s, coef;  // coef = 1 / (B * sqrt(hd_s))
};
__global__ __launch_bounds__(256) void rel_grad_kernel(const RelGradArgs a) {
  // one wave per Gram row, four columns per lane: 16-byte loads of both Grams, one 8-byte (bf16) or 16-byte store
  const int b = blockIdx.y, i = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int j0 = (threadIdx.x & 63) * 4;  // ldr == 256
  const size_t o = ((size_t)b * a.ldr + i) * a.ldr + j0;
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (i < a.N) {
    const float up = (a.upstream ? *a.upstream : 1.0f) * a.coef;
    const f32x4 rsv = *(const f32x4*)(a.rs + o), rtv = *(const f32x4*)(a.rt + o);
    const float lsi = a.lse_s[b * a.N + i], lti = a.lse_t[b * a.N + i];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int j = j0 + e;
      if (j < a.N) {
        const float rs = rsv[e] * a.inv_sqrt_s, rt = rtv[e] * a.inv_sqrt_t;
        const float lsj = a.lse_s[b * a.N + j], ltj = a.lse_t[b * a.N + j];
        v[e] = (expf(rs - lsi) + expf(rs - lsj) - expf(rt - lti) - expf(rt - ltj)) * up;
      }
    }
  }
  if (a.out_f32) *(f32x4*)((float*)a.S + o) = v;
  else {
    const bf16x4 ob = {f2bf(v[0]), f2bf(v[1]), f2bf(v[2]), f2bf(v[3])};
    *(bf16x4*)((__bf16*)a.S + o) = ob;
  }
}

// ---- token MSE (nn.MSELoss, utils/losses.py:194,228,241-242): loss (+)= mean((a-b)^2), da = 2 (a-b) / n ---------
__global__ __launch_bounds__(1024) void mse_kernel(const float* a, const float* b, size_t n, float* loss, float* da,
                                                   int accumulate) {
  __shared__ float red[16];
  float s = 0.f;
  const float inv = 1.0f / (float)n;
  for (size_t i = threadIdx.x; i < n; i += 1024) {
    const float d = a[i] - b[i];
    s += d * d;
    if (da) da[i] = 2.0f * d * inv;
  }
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = 0.f;
    for (int i = 0; i < 16; ++i) t += red[i];
    loss[0] = (accumulate ? loss[0] : 0.f) + t * inv;
  }
}

// ---- token KL (nn.KLDivLoss(reduction="batchmean", log_target=True), utils/losses.py:192-193,228,241-242): student tokens s and teacher tokens t
//      are read as log-probabilities as they stand: loss (+)= sum e^t (t - s) / batch, ds = -e^t / batch (independent of s).  Nothing is
//      clamped: a non-finite token gives the non-finite loss torch gives.  One block, fixed summation order, as mse_kernel.
__global__ __launch_bounds__(1024) void kldiv_kernel(const float* s, const float* t, size_t n, float batch, float* loss, float* ds,
                                                     int accumulate) {
  __shared__ float red[16];
  float acc = 0.f;
  for (size_t i = threadIdx.x; i < n; i += 1024) {
    const float tv = t[i];
    const float e = expf(tv);
    acc += e * (tv - s[i]);
    if (ds) ds[i] = -e / batch;
  }
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    float r = 0.f;
    for (int i = 0; i < 16; ++i) r += red[i];
    loss[0] = (accumulate ? loss[0] : 0.f) + r / batch;
  }
}

}  // namespace

extern "C" int devit_token_mse(const float* a, const float* b, size_t n, float* loss, float* da, int accumulate,
                               void* stream) {
  DEVIT_CHECK(a && b && loss && n > 0, DEVIT_ERR_ARG, "devit_token_mse: bad argument");
  hipLaunchKernelGGL(mse_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, a, b, n, loss, da, accumulate);
  DEVIT_LAUNCH_CHECK();
  return DEVIT_OK;
}

extern "C" int devit_token_kldiv(const float* s, const float* t, size_t n, int batch, float* loss, float* ds, int accumulate,
                                 void* stream) {
  DEVIT_CHECK(s && t && loss && n > 0, DEVIT_ERR_ARG, "devit_token_kldiv: bad argument");
  DEVIT_CHECK(batch > 0 && n % (size_t)batch == 0, DEVIT_ERR_SHAPE, "devit_token_kldiv: batch=%d must be positive and divide n=%zu", batch, n);
  hipLaunchKernelGGL(kldiv_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, s, t, n, (float)batch, loss, ds, accumulate);
  DEVIT_LAUNCH_CHECK();
  return DEVIT_OK;
}

extern "C" int devit_cls_distill_loss(const float* logits, const float* logits_kd, const float* teacher_logits,
                                      const float* soft_targets, int B, int C, int kind, float alpha, float tau,
                                      float* loss3, float* dlogits, float* dlogits_kd, void* stream) {
  DEVIT_CHECK(logits && logits_kd && soft_targets && loss3 && dlogits && dlogits_kd, DEVIT_ERR_ARG,
              "devit_cls_distill_loss: null pointer");
  DEVIT_CHECK(kind == 0 || teacher_logits, DEVIT_ERR_ARG, "devit_cls_distill_loss: teacher logits required");
  DEVIT_CHECK(B > 0 && C > 0 && C <= 64 * MAXC_PER_LANE && kind >= 0 && kind <= 2, DEVIT_ERR_SHAPE,
              "devit_cls_distill_loss: C=%d must be <= 1024", C);
  ClsArgs a{logits, logits_kd, teacher_logits, soft_targets, loss3, dlogits, dlogits_kd, B, C, kind, alpha, tau};
  hipError_t me = hipMemsetAsync(loss3, 0, 3 * sizeof(float), (hipStream_t)stream);
  DEVIT_CHECK(me == hipSuccess, DEVIT_ERR_LAUNCH, "devit_cls_distill_loss: hipMemsetAsync: %s", hipGetErrorString(me));
  const int groups = (B + 15) / 16;
  if (groups > 1 && devit_det::on()) {   // deterministic mode (det.h): the workgroups' shares go to the workspace and are added to the scalars in workgroup order
    float* ws = nullptr;
    const int rc = devit_det::workspace("devit_cls_distill_loss", (size_t)groups * 3 * sizeof(float), &ws);
    if (rc != DEVIT_OK) return rc;
    a.loss = ws;
    hipLaunchKernelGGL(cls_loss_det_kernel, dim3(groups), dim3(1024), 0, (hipStream_t)stream, a);
    DEVIT_LAUNCH_CHECK();
    return devit_det::fold(ws, groups, 3, 1, 3, loss3, 0, 1, 0, (hipStream_t)stream);
  }
  hipLaunchKernelGGL(cls_loss_kernel, dim3(groups), dim3(1024), 0, (hipStream_t)stream, a);
  DEVIT_LAUNCH_CHECK();
  return DEVIT_OK;
}

extern "C" int devit_relation_stats(const float* gram_t, const float* gram_s, int B, int N, int ldr, int head_dim_t,
                                    int head_dim_s, float* lse_t, float* lse_s, float* row_kl, float* loss,
                                    void* stream) {
  DEVIT_CHECK(gram_t && gram_s && lse_t && lse_s && row_kl && loss, DEVIT_ERR_ARG, "devit_relation_stats: null pointer");
  DEVIT_CHECK(N > 0 && N <= 256 && ldr >= N && ldr <= 256 && ldr % 4 == 0, DEVIT_ERR_SHAPE,
              "devit_relation_stats: N=%d must be <= ldr=%d <= 256, ldr a multiple of 4", N, ldr);
  RelStatArgs a{gram_t, gram_s, lse_t, lse_s, row_kl, B, N, ldr, 1.0f / sqrtf((float)head_dim_t),
                1.0f / sqrtf((float)head_dim_s)};
  hipLaunchKernelGGL(rel_stats_kernel, dim3((B * N + 3) / 4), dim3(256), 0, (hipStream_t)stream, a);
  DEVIT_LAUNCH_CHECK();
  hipLaunchKernelGGL(fixed_order_reduce_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, (const float*)row_kl, (long long)B * N,
                     1.0f / (float)B, loss);
  DEVIT_LAUNCH_CHECK();
  return DEVIT_OK;
}

extern "C" int devit_relation_grad(const float* gram_t, const float* gram_s, const float* lse_t, const float* lse_s,
                                   const float* upstream, int B, int N, int ldr, int head_dim_t, int head_dim_s,
                                   void* S_out, int out_is_f32, void* stream) {
  DEVIT_CHECK(gram_t && gram_s && lse_t && lse_s && S_out, DEVIT_ERR_ARG, "devit_relation_grad: null pointer");
  DEVIT_CHECK(ldr == 256 && N <= 256, DEVIT_ERR_SHAPE, "devit_relation_grad: padded Gram must be 256 wide");
  RelGradArgs a{gram_t, gram_s, lse_t, lse_s, upstream, S_out, B, N, ldr, out_is_f32,
                1.0f / sqrtf((float)head_dim_t), 1.0f / sqrtf((float)head_dim_s),
                1.0f / ((float)B * sqrtf((float)head_dim_s))};
  hipLaunchKernelGGL(rel_grad_kernel, dim3(ldr / 4, B), dim3(256), 0, (hipStream_t)stream, a);
  DEVIT_LAUNCH_CHECK();
  return DEVIT_OK;
}
