// The optimizer of the flat parameter buffer: the squared gradient norm (devit_sumsq_f32) and the five fused tails of `--opt` -- AdamW,
// SGD with momentum (plain and Nesterov), Adam with L2 decay coupled into the gradient, and LAMB with per-tensor trust ratios: timm 0.5.4's
// `adamw`, `momentum`, `nesterov`, `adam`, `lamb` / `lambc` (create_optimizer, distill_sub.py:340).  One frame, written once: the arguments
// (OptArgs), the global-norm clip folded into the gradient load (tail_clip), the per-granule weight decay exemption, the EMA and the bf16
// re-cast of the new weights (model_tail), and on the host one validation + fill (fill_args) and one launch (launch_tail).  A tail adds its
// update rule between the two.  All of them are HBM-bound streams: one thread owns a 16-byte granule of every buffer, loads and stores are 16
// bytes wide.  Every tail has a sibling with a learning rate per granule (the *_lrs kernels, LrScale): lr = dyn[0] * lr_scales[lr_group4[granule]].
#include "devit_common.h"

namespace {

struct OptArgs {
  float* p; const float* g; float* m; float* v; float* ema; __bf16* p_bf16;   // m: the momentum buffer of SGD; v unused there
  const float* gnorm_sq;            // device scalar: sum of squared grads (NULL = no clipping; LAMB always needs it)
  const float* dyn;                 // device: lr (SGD) or lr, 1 - beta1^step, 1 - beta2^step
  const unsigned char* no_decay4;   // one byte per granule: != 0 -> no weight decay there (NULL: decay all)
  size_t n;
  float beta1, beta2, eps, wd, max_norm, ema_decay, grad_scale;   // beta1: the momentum of SGD
  int nesterov;
};

// grad_scale * min(1, max_norm / (||g|| * grad_scale + 1e-6)): timm NativeScaler's clip_grad_norm_ and the mean of DDP, every tail's first line
__device__ __forceinline__ float tail_clip(const float* gnorm_sq, float max_norm, float grad_scale) {
  float clip = grad_scale;
  if (gnorm_sq) {
    const float nrm = sqrtf(*gnorm_sq) * grad_scale;
    const float c = max_norm / (nrm + 1e-6f);   // torch.nn.utils.clip_grad_norm_
    clip *= c < 1.0f ? c : 1.0f;
  }
  return clip;
}

// ema = ema*d + (1-d)*p and p_bf16 = bf16(p) for one granule (both optional)
__device__ __forceinline__ void model_tail(float* ema, __bf16* p_bf16, size_t i, f32x4 p, float ema_decay) {
  if (ema) {
    f32x4 e = *(const f32x4*)(ema + i * 4);
    e = e * ema_decay + (1.0f - ema_decay) * p;
    *(f32x4*)(ema + i * 4) = e;
  }
  if (p_bf16) {
    bf16x4 ob = {f2bf(p[0]), f2bf(p[1]), f2bf(p[2]), f2bf(p[3])};
    *(bf16x4*)(p_bf16 + i * 4) = ob;
  }
}

// ---- torch.optim.AdamW + timm NativeScaler clip_grad_norm_ + timm ModelEma.update (engine.py:127,131-132): the decay is decoupled,
// p *= 1 - lr wd on the granules that are not exempt; dyn (lr, 1 - beta1^step, 1 - beta2^step) changes every step and is graph-safe
__global__ __launch_bounds__(256) void adamw_kernel(const OptArgs a) {
  const float clip = tail_clip(a.gnorm_sq, a.max_norm, a.grad_scale);
  const float lr = a.dyn[0], bc1 = a.dyn[1], bc2 = a.dyn[2];
  const size_t n4 = a.n / 4;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
    f32x4 p = *(const f32x4*)(a.p + i * 4);
    const f32x4 g = *(const f32x4*)(a.g + i * 4) * clip;
    f32x4 m = *(const f32x4*)(a.m + i * 4), v = *(const f32x4*)(a.v + i * 4);
    if (!(a.no_decay4 && a.no_decay4[i])) p *= (1.0f - lr * a.wd);
    m = a.beta1 * m + (1.0f - a.beta1) * g;
    v = a.beta2 * v + (1.0f - a.beta2) * g * g;
#pragma unroll
    for (int e = 0; e < 4; ++e) p[e] -= (lr / bc1) * m[e] / (sqrtf(v[e]) / sqrtf(bc2) + a.eps);
    *(f32x4*)(a.p + i * 4) = p;
    *(f32x4*)(a.m + i * 4) = m;
    *(f32x4*)(a.v + i * 4) = v;
    model_tail(a.ema, a.p_bf16, i, p, a.ema_decay);
  }
}

// ---- torch.optim.SGD(momentum = mu, nesterov, dampening = 0): d = g' + wd p;  buf' = mu buf + d;  p' = p - lr (nesterov ? d + mu buf' : buf')
// buf starts at zero, which is torch's first step (buf = d).
__global__ __launch_bounds__(256) void sgd_kernel(const OptArgs a) {
  const float clip = tail_clip(a.gnorm_sq, a.max_norm, a.grad_scale);
  const float lr = a.dyn[0], mu = a.beta1;
  const size_t n4 = a.n / 4;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
    f32x4 p = *(const f32x4*)(a.p + i * 4);
    const f32x4 g = *(const f32x4*)(a.g + i * 4) * clip;
    f32x4 buf = *(const f32x4*)(a.m + i * 4);
    const float wd = (a.no_decay4 && a.no_decay4[i]) ? 0.0f : a.wd;
    const f32x4 d = g + wd * p;
    buf = mu * buf + d;
    p -= lr * (a.nesterov ? d + mu * buf : buf);
    *(f32x4*)(a.p + i * 4) = p;
    *(f32x4*)(a.m + i * 4) = buf;
    model_tail(a.ema, a.p_bf16, i, p, a.ema_decay);
  }
}

// ---- torch.optim.Adam: the decay enters the gradient (d = g' + wd p) and with it both moments; the update is adamw_kernel's, without its p *= 1 - lr wd
__global__ __launch_bounds__(256) void adam_l2_kernel(const OptArgs a) {
  const float clip = tail_clip(a.gnorm_sq, a.max_norm, a.grad_scale);
  const float lr = a.dyn[0], bc1 = a.dyn[1], bc2 = a.dyn[2];
  const size_t n4 = a.n / 4;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
    f32x4 p = *(const f32x4*)(a.p + i * 4);
    const f32x4 g = *(const f32x4*)(a.g + i * 4) * clip;
    f32x4 m = *(const f32x4*)(a.m + i * 4), v = *(const f32x4*)(a.v + i * 4);
    const float wd = (a.no_decay4 && a.no_decay4[i]) ? 0.0f : a.wd;
    const f32x4 d = g + wd * p;
    m = a.beta1 * m + (1.0f - a.beta1) * d;
    v = a.beta2 * v + (1.0f - a.beta2) * d * d;
#pragma unroll
    for (int e = 0; e < 4; ++e) p[e] -= (lr / bc1) * m[e] / (sqrtf(v[e]) / sqrtf(bc2) + a.eps);
    *(f32x4*)(a.p + i * 4) = p;
    *(f32x4*)(a.m + i * 4) = m;
    *(f32x4*)(a.v + i * 4) = v;
    model_tail(a.ema, a.p_bf16, i, p, a.ema_decay);
  }
}

// ---- the three tails above with a learning rate per granule (layer-wise lr decay): lr = dyn[0] * scales[group4[i]], one fp32 multiply, used
// wherever the sibling uses lr.  scales has 256 entries, so the byte needs no check: no address depends on what the array holds.  The byte is
// a 64-byte load per wave like no_decay4's; the table is a gather of one dword per lane through the vector cache, where its 1 KB (eight
// 128-byte lines, re-read by every wave) stays; a wave's 64 granules lie in one tensor or two, so a gather touches one or two lines.
struct LrScale {
  const unsigned char* group4;      // one byte per granule: the index of its scale
  const float* scales;              // [256]
};

__global__ __launch_bounds__(256) void adamw_lrs_kernel(const OptArgs a, const LrScale s) {
  const float clip = tail_clip(a.gnorm_sq, a.max_norm, a.grad_scale);
  const float lr0 = a.dyn[0], bc1 = a.dyn[1], bc2 = a.dyn[2];
  const size_t n4 = a.n / 4;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
    const float lr = lr0 * s.scales[s.group4[i]];
    f32x4 p = *(const f32x4*)(a.p + i * 4);
    const f32x4 g = *(const f32x4*)(a.g + i * 4) * clip;
    f32x4 m = *(const f32x4*)(a.m + i * 4), v = *(const f32x4*)(a.v + i * 4);
    if (!(a.no_decay4 && a.no_decay4[i])) p *= (1.0f - lr * a.wd);
    m = a.beta1 * m + (1.0f - a.beta1) * g;
    v = a.beta2 * v + (1.0f - a.beta2) * g * g;
#pragma unroll
    for (int e = 0; e < 4; ++e) p[e] -= (lr / bc1) * m[e] / (sqrtf(v[e]) / sqrtf(bc2) + a.eps);
    *(f32x4*)(a.p + i * 4) = p;
    *(f32x4*)(a.m + i * 4) = m;
    *(f32x4*)(a.v + i * 4) = v;
    model_tail(a.ema, a.p_bf16, i, p, a.ema_decay);
  }
}

__global__ __launch_bounds__(256) void sgd_lrs_kernel(const OptArgs a, const LrScale s) {
  const float clip = tail_clip(a.gnorm_sq, a.max_norm, a.grad_scale);
  const float lr0 = a.dyn[0], mu = a.beta1;
  const size_t n4 = a.n / 4;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
    const float lr = lr0 * s.scales[s.group4[i]];
    f32x4 p = *(const f32x4*)(a.p + i * 4);
    const f32x4 g = *(const f32x4*)(a.g + i * 4) * clip;
    f32x4 buf = *(const f32x4*)(a.m + i * 4);
    const float wd = (a.no_decay4 && a.no_decay4[i]) ? 0.0f : a.wd;
    const f32x4 d = g + wd * p;
    buf = mu * buf + d;
    p -= lr * (a.nesterov ? d + mu * buf : buf);
    *(f32x4*)(a.p + i * 4) = p;
    *(f32x4*)(a.m + i * 4) = buf;
    model_tail(a.ema, a.p_bf16, i, p, a.ema_decay);
  }
}

__global__ __launch_bounds__(256) void adam_l2_lrs_kernel(const OptArgs a, const LrScale s) {
  const float clip = tail_clip(a.gnorm_sq, a.max_norm, a.grad_scale);
  const float lr0 = a.dyn[0], bc1 = a.dyn[1], bc2 = a.dyn[2];
  const size_t n4 = a.n / 4;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
    const float lr = lr0 * s.scales[s.group4[i]];
    f32x4 p = *(const f32x4*)(a.p + i * 4);
    const f32x4 g = *(const f32x4*)(a.g + i * 4) * clip;
    f32x4 m = *(const f32x4*)(a.m + i * 4), v = *(const f32x4*)(a.v + i * 4);
    const float wd = (a.no_decay4 && a.no_decay4[i]) ? 0.0f : a.wd;
    const f32x4 d = g + wd * p;
    m = a.beta1 * m + (1.0f - a.beta1) * d;
    v = a.beta2 * v + (1.0f - a.beta2) * d * d;
#pragma unroll
    for (int e = 0; e < 4; ++e) p[e] -= (lr / bc1) * m[e] / (sqrtf(v[e]) / sqrtf(bc2) + a.eps);
    *(f32x4*)(a.p + i * 4) = p;
    *(f32x4*)(a.m + i * 4) = m;
    *(f32x4*)(a.v + i * 4) = v;
    model_tail(a.ema, a.p_bf16, i, p, a.ema_decay);
  }
}

// ---- LAMB (timm Lamb: bias_correction, grad_averaging, max_grad_norm = 1, always_adapt = False) ---------------------------------
// The trust ratio ||p|| / ||u|| is per PARAMETER TENSOR, so the flat buffer is cut into chunks (devit_opt_chunk: at most
// LAMB_CHUNK4 granules of ONE tensor), one workgroup each:
//   lamb_moments_kernel  m', v' stored; u formed; per chunk of a decayed tensor (sum p^2, sum u^2) -> partials[chunk]
//   lamb_trust_kernel    one wave per tensor adds its chunks' partials in a fixed order -> trust[tensor]
//   lamb_apply_kernel    u recomputed from p, m', v' (lamb_update, the function phase 1 used), p' = p - lr trust u, EMA, bf16 copy
// No float atomics: every sum has one order, two runs give the same bits.  Tensors of the no-decay group take trust = 1
// without a norm (always_adapt is off).
constexpr unsigned LAMB_CHUNK4 = 1024;
constexpr int CHUNK_NO_DECAY = 1;

// u = (m' / bc1) / (sqrt(v') / sqrt(bc2) + eps) + wd p, every operation rounded on its own so that phases 1 and 3 agree to the bit
__device__ __forceinline__ f32x4 lamb_update(f32x4 p, f32x4 m, f32x4 v, float bc1, float sqrt_bc2, float eps, float wd) {
#pragma clang fp contract(off)
  f32x4 u;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float r = (m[e] / bc1) / (sqrtf(v[e]) / sqrt_bc2 + eps);
    u[e] = r + wd * p[e];
  }
  return u;
}

struct LambArgs {
  OptArgs o;
  const devit_opt_chunk* chunks;
  float* partials;   // [nchunks][2]: sum p^2, sum u^2 (chunks of decayed tensors only)
  float* trust;      // [nsegments]
  int nchunks, nsegments, trust_clip;
};

// a chunk the kernels may address: inside the buffer, at most LAMB_CHUNK4 granules, a segment the trust array has.  The host
// validates the whole table before it uploads it (optim.validate_chunk_table); this keeps even a corrupted one inside the buffers.
__device__ __forceinline__ bool chunk_ok(const devit_opt_chunk c, size_t n4, int nsegments) {
  return c.count4 <= LAMB_CHUNK4 && (size_t)c.first4 + c.count4 <= n4 && c.segment >= 0 && c.segment < nsegments;
}

__global__ __launch_bounds__(256) void lamb_moments_kernel(const LambArgs a) {
  __shared__ float red[2][4];
  const devit_opt_chunk c = a.chunks[blockIdx.x];
  if (!chunk_ok(c, a.o.n / 4, a.nsegments)) return;
  float clip = tail_clip(a.o.max_norm > 0.0f ? a.o.gnorm_sq : nullptr, a.o.max_norm, a.o.grad_scale);
  const float n1 = sqrtf(*a.o.gnorm_sq) * clip;        // the norm of the gradients the optimizer sees
  if (n1 > 1.0f) clip = clip / n1;                     // timm Lamb's own max_grad_norm = 1.0, on top of --clip-grad
  const float bc1 = a.o.dyn[1], sqrt_bc2 = sqrtf(a.o.dyn[2]);
  const bool decayed = !(c.flags & CHUNK_NO_DECAY);
  const float wd = decayed ? a.o.wd : 0.0f;
  float sp = 0.f, su = 0.f;
  for (unsigned t = threadIdx.x; t < c.count4; t += 256) {
    const size_t i = (size_t)c.first4 + t;
    const f32x4 p = *(const f32x4*)(a.o.p + i * 4);
    const f32x4 g = *(const f32x4*)(a.o.g + i * 4) * clip;
    f32x4 m = *(const f32x4*)(a.o.m + i * 4), v = *(const f32x4*)(a.o.v + i * 4);
    m = a.o.beta1 * m + (1.0f - a.o.beta1) * g;
    v = a.o.beta2 * v + (1.0f - a.o.beta2) * g * g;
    *(f32x4*)(a.o.m + i * 4) = m;
    *(f32x4*)(a.o.v + i * 4) = v;
    if (decayed) {
      const f32x4 u = lamb_update(p, m, v, bc1, sqrt_bc2, a.o.eps, wd);
      sp += p[0] * p[0] + p[1] * p[1] + p[2] * p[2] + p[3] * p[3];
      su += u[0] * u[0] + u[1] * u[1] + u[2] * u[2] + u[3] * u[3];
    }
  }
  if (!decayed) return;                                // block-uniform
  sp = wave_sum(sp);
  su = wave_sum(su);
  if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = sp; red[1][threadIdx.x >> 6] = su; }
  __syncthreads();
  if (threadIdx.x == 0) {
    const f32x2 out = {red[0][0] + red[0][1] + red[0][2] + red[0][3], red[1][0] + red[1][1] + red[1][2] + red[1][3]};
    *(f32x2*)(a.partials + (size_t)blockIdx.x * 2) = out;
  }
}

// one wave per tensor.  The table is sorted by segment (validated on the host): the tensor's chunks are one run, found by a
// lower-bound search; lane l adds chunks l, l + 64, ... of the run, then the wave sums.
__global__ __launch_bounds__(64) void lamb_trust_kernel(const LambArgs a) {
  const int seg = blockIdx.x;
  int lo = 0, hi = a.nchunks;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (a.chunks[mid].segment < seg) lo = mid + 1; else hi = mid;
  }
  float sp = 0.f, su = 0.f;
  bool decayed = false;
  if (lo < a.nchunks && a.chunks[lo].segment == seg && !(a.chunks[lo].flags & CHUNK_NO_DECAY)) {
    decayed = true;
    for (int ch = lo + (int)threadIdx.x; ch < a.nchunks && a.chunks[ch].segment == seg; ch += 64) {
      const f32x2 v = *(const f32x2*)(a.partials + (size_t)ch * 2);
      sp += v[0];
      su += v[1];
    }
  }
  sp = wave_sum(sp);
  su = wave_sum(su);
  if (threadIdx.x == 0) {
    float t = 1.0f;
    if (decayed) {
      const float wn = sqrtf(sp), un = sqrtf(su);
      if (wn > 0.0f && un > 0.0f) t = wn / un;
      if (a.trust_clip && t > 1.0f) t = 1.0f;
    }
    a.trust[seg] = t;
  }
}

__global__ __launch_bounds__(256) void lamb_apply_kernel(const LambArgs a) {
  const devit_opt_chunk c = a.chunks[blockIdx.x];
  if (!chunk_ok(c, a.o.n / 4, a.nsegments)) return;
  const float lr = a.o.dyn[0], bc1 = a.o.dyn[1], sqrt_bc2 = sqrtf(a.o.dyn[2]);
  const float wd = (c.flags & CHUNK_NO_DECAY) ? 0.0f : a.o.wd;
  const float step = lr * a.trust[c.segment];
  for (unsigned t = threadIdx.x; t < c.count4; t += 256) {
    const size_t i = (size_t)c.first4 + t;
    f32x4 p = *(const f32x4*)(a.o.p + i * 4);
    const f32x4 m = *(const f32x4*)(a.o.m + i * 4), v = *(const f32x4*)(a.o.v + i * 4);
    p -= step * lamb_update(p, m, v, bc1, sqrt_bc2, a.o.eps, wd);
    *(f32x4*)(a.o.p + i * 4) = p;
    model_tail(a.o.ema, a.o.p_bf16, i, p, a.o.ema_decay);
  }
}

// lamb_apply_kernel with the learning rate per granule: p' = p - (lr scale) trust u.  The moments and the trust ratio do not see the scale.
__global__ __launch_bounds__(256) void lamb_apply_lrs_kernel(const LambArgs a, const LrScale s) {
  const devit_opt_chunk c = a.chunks[blockIdx.x];
  if (!chunk_ok(c, a.o.n / 4, a.nsegments)) return;
  const float lr0 = a.o.dyn[0], bc1 = a.o.dyn[1], sqrt_bc2 = sqrtf(a.o.dyn[2]);
  const float wd = (c.flags & CHUNK_NO_DECAY) ? 0.0f : a.o.wd;
  const float trust = a.trust[c.segment];
  for (unsigned t = threadIdx.x; t < c.count4; t += 256) {
    const size_t i = (size_t)c.first4 + t;
    const float step = (lr0 * s.scales[s.group4[i]]) * trust;
    f32x4 p = *(const f32x4*)(a.o.p + i * 4);
    const f32x4 m = *(const f32x4*)(a.o.m + i * 4), v = *(const f32x4*)(a.o.v + i * 4);
    p -= step * lamb_update(p, m, v, bc1, sqrt_bc2, a.o.eps, wd);
    *(f32x4*)(a.o.p + i * 4) = p;
    model_tail(a.o.ema, a.o.p_bf16, i, p, a.o.ema_decay);
  }
}

// ---- sum of squares of a flat f32 buffer -> out[0] (two-stage, deterministic): the norm tail_clip reads
__global__ __launch_bounds__(256) void sumsq_stage1(const float* g, size_t n, float* partial) {
  __shared__ float red[4];
  float s = 0.f;
  const size_t n4 = n / 4;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
    const f32x4 v = *(const f32x4*)(g + i * 4);
    s += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
  }
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}
__global__ __launch_bounds__(256) void sumsq_stage2(const float* partial, int n, float* out) {
  __shared__ float red[4];
  float s = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) s += partial[i];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) out[0] = red[0] + red[1] + red[2] + red[3];
}

inline int grid_for(size_t work_items, int cap) {
  size_t g = (work_items + 255) / 256;
  return (int)(g < 1 ? 1 : (g > (size_t)cap ? cap : g));
}

// every entry point's argument check and fill: `who` names it in the messages; v is required where the tail keeps two moments
int fill_args(OptArgs& a, const char* who, bool two_moments, float* p, const float* g, float* m, float* v, float* ema, void* p_bf16,
              const unsigned char* no_decay4, const float* gnorm_sq, const float* dyn, size_t n, float beta1, float beta2, float eps,
              float weight_decay, float max_norm, float ema_decay, float grad_scale, int nesterov) {
  DEVIT_CHECK(p && g && m && (v || !two_moments) && dyn, DEVIT_ERR_ARG, "%s: bad argument", who);
  DEVIT_CHECK(n % 4 == 0, DEVIT_ERR_SHAPE, "%s: n must be a multiple of 4 (pad the flat buffer)", who);
  a.p = p; a.g = g; a.m = m; a.v = v; a.ema = ema; a.p_bf16 = (__bf16*)p_bf16; a.gnorm_sq = gnorm_sq; a.dyn = dyn;
  a.no_decay4 = no_decay4; a.n = n; a.beta1 = beta1; a.beta2 = beta2; a.eps = eps; a.wd = weight_decay;
  a.max_norm = max_norm; a.ema_decay = ema_decay; a.grad_scale = grad_scale; a.nesterov = nesterov != 0;
  return DEVIT_OK;
}

// a grid-stride tail: one thread per granule up to 4096 workgroups
int launch_tail(void (*kernel)(const OptArgs), const OptArgs& a, void* stream) {
  hipLaunchKernelGGL(kernel, dim3(grid_for(a.n / 4, 4096)), dim3(256), 0, (hipStream_t)stream, a);
  DEVIT_LAUNCH_CHECK();
  return DEVIT_OK;
}

// the same launch for a tail with a learning rate per granule: both arrays are required (a caller without scales has the sibling entry point)
int launch_tail(void (*kernel)(const OptArgs, const LrScale), const OptArgs& a, const char* who, const unsigned char* lr_group4,
                const float* lr_scales, void* stream) {
  DEVIT_CHECK(lr_group4 && lr_scales, DEVIT_ERR_ARG, "%s: lr_group4 (n / 4 bytes) and lr_scales (256 floats) are required", who);
  const LrScale s = {lr_group4, lr_scales};
  hipLaunchKernelGGL(kernel, dim3(grid_for(a.n / 4, 4096)), dim3(256), 0, (hipStream_t)stream, a, s);
  DEVIT_LAUNCH_CHECK();
  return DEVIT_OK;
}

}  // namespace

extern "C" size_t devit_sumsq_workspace(void) { return 1024 * sizeof(float); }

extern "C" int devit_sumsq_f32(const float* g, size_t n, float* out, void* workspace, size_t workspace_bytes,
                               void* stream) {
  DEVIT_CHECK(g && out && workspace && workspace_bytes >= 1024 * sizeof(float), DEVIT_ERR_ARG, "devit_sumsq_f32: bad argument");
  DEVIT_CHECK(n % 4 == 0, DEVIT_ERR_SHAPE, "devit_sumsq_f32: n must be a multiple of 4 (pad the flat buffer)");
  hipLaunchKernelGGL(sumsq_stage1, dim3(1024), dim3(256), 0, (hipStream_t)stream, g, n, (float*)workspace);
  DEVIT_LAUNCH_CHECK();
  hipLaunchKernelGGL(sumsq_stage2, dim3(1), dim3(256), 0, (hipStream_t)stream, (const float*)workspace, 1024, out);
  DEVIT_LAUNCH_CHECK();
  return DEVIT_OK;
}

extern "C" int devit_adamw_step(float* p, const float* g, float* m, float* v, float* ema, void* p_bf16,
                                const unsigned char* no_decay4, const float* gnorm_sq, const float* dyn, size_t n,
                                float beta1, float beta2, float eps, float weight_decay, float max_norm, float ema_decay,
                                float grad_scale, void* stream) {
  OptArgs a;
  if (int rc = fill_args(a, "devit_adamw_step", true, p, g, m, v, ema, p_bf16, no_decay4, gnorm_sq, dyn, n, beta1, beta2, eps,
                         weight_decay, max_norm, ema_decay, grad_scale, 0))
    return rc;
  return launch_tail(adamw_kernel, a, stream);
}

extern "C" int devit_sgd_step(float* p, const float* g, float* buf, float* ema, void* p_bf16, const unsigned char* no_decay4,
                              const float* gnorm_sq, const float* dyn, size_t n, float momentum, int nesterov,
                              float weight_decay, float max_norm, float ema_decay, float grad_scale, void* stream) {
  OptArgs a;
  if (int rc = fill_args(a, "devit_sgd_step", false, p, g, buf, nullptr, ema, p_bf16, no_decay4, gnorm_sq, dyn, n, momentum, 0.0f, 0.0f,
                         weight_decay, max_norm, ema_decay, grad_scale, nesterov))
    return rc;
  return launch_tail(sgd_kernel, a, stream);
}

extern "C" int devit_adam_l2_step(float* p, const float* g, float* m, float* v, float* ema, void* p_bf16,
                                  const unsigned char* no_decay4, const float* gnorm_sq, const float* dyn, size_t n,
                                  float beta1, float beta2, float eps, float weight_decay, float max_norm, float ema_decay,
                                  float grad_scale, void* stream) {
  OptArgs a;
  if (int rc = fill_args(a, "devit_adam_l2_step", true, p, g, m, v, ema, p_bf16, no_decay4, gnorm_sq, dyn, n, beta1, beta2, eps,
                         weight_decay, max_norm, ema_decay, grad_scale, 0))
    return rc;
  return launch_tail(adam_l2_kernel, a, stream);
}

extern "C" size_t devit_lamb_workspace(int nchunks, int nsegments) {
  if (nchunks < 0 || nsegments < 0) return 0;
  return ((size_t)nchunks * 2 + (size_t)nsegments) * sizeof(float);
}

// devit_lamb_step and devit_lamb_step_lrs (`scaled`: the last launch is lamb_apply_lrs_kernel over lr_group4 / lr_scales, both required)
static int lamb_step(const char* who, bool scaled, float* p, const float* g, float* m, float* v, float* ema, void* p_bf16,
                     const float* gnorm_sq, const float* dyn, size_t n, const devit_opt_chunk* chunks, int nchunks, int nsegments,
                     int trust_clip, float beta1, float beta2, float eps, float weight_decay, float max_norm, float ema_decay,
                     float grad_scale, void* workspace, size_t workspace_bytes, const unsigned char* lr_group4, const float* lr_scales,
                     void* stream) {
  DEVIT_CHECK(p && g && m && v && dyn && gnorm_sq && chunks && workspace, DEVIT_ERR_ARG,
              "%s: bad argument (gnorm_sq is required: LAMB clips the gradient to norm 1 itself)", who);
  DEVIT_CHECK(!scaled || (lr_group4 && lr_scales), DEVIT_ERR_ARG, "%s: lr_group4 (n / 4 bytes) and lr_scales (256 floats) are required", who);
  LambArgs a;
  if (int rc = fill_args(a.o, who, true, p, g, m, v, ema, p_bf16, nullptr, gnorm_sq, dyn, n, beta1, beta2, eps, weight_decay,
                         max_norm, ema_decay, grad_scale, 0))
    return rc;
  DEVIT_CHECK(nchunks > 0 && nsegments > 0 && n / 4 <= 0xffffffffu, DEVIT_ERR_SHAPE,
              "%s: nchunks = %d, nsegments = %d must be positive, n / 4 must fit 32 bits", who, nchunks, nsegments);
  DEVIT_CHECK(workspace_bytes >= devit_lamb_workspace(nchunks, nsegments) && ((size_t)workspace & 7) == 0, DEVIT_ERR_ARG,
              "%s: workspace of %zu bytes, devit_lamb_workspace(%d, %d) = %zu (8-byte aligned)", who, workspace_bytes,
              nchunks, nsegments, devit_lamb_workspace(nchunks, nsegments));
  a.chunks = chunks; a.nchunks = nchunks; a.nsegments = nsegments; a.trust_clip = trust_clip != 0;
  a.partials = (float*)workspace;
  a.trust = a.partials + (size_t)nchunks * 2;
  hipLaunchKernelGGL(lamb_moments_kernel, dim3(nchunks), dim3(256), 0, (hipStream_t)stream, a);
  DEVIT_LAUNCH_CHECK();
  hipLaunchKernelGGL(lamb_trust_kernel, dim3(nsegments), dim3(64), 0, (hipStream_t)stream, a);
  DEVIT_LAUNCH_CHECK();
  if (scaled) {
    const LrScale s = {lr_group4, lr_scales};
    hipLaunchKernelGGL(lamb_apply_lrs_kernel, dim3(nchunks), dim3(256), 0, (hipStream_t)stream, a, s);
  } else {
    hipLaunchKernelGGL(lamb_apply_kernel, dim3(nchunks), dim3(256), 0, (hipStream_t)stream, a);
  }
  DEVIT_LAUNCH_CHECK();
  return DEVIT_OK;
}

extern "C" int devit_lamb_step(float* p, const float* g, float* m, float* v, float* ema, void* p_bf16, const float* gnorm_sq,
                               const float* dyn, size_t n, const devit_opt_chunk* chunks, int nchunks, int nsegments,
                               int trust_clip, float beta1, float beta2, float eps, float weight_decay, float max_norm,
                               float ema_decay, float grad_scale, void* workspace, size_t workspace_bytes, void* stream) {
  return lamb_step("devit_lamb_step", false, p, g, m, v, ema, p_bf16, gnorm_sq, dyn, n, chunks, nchunks, nsegments, trust_clip, beta1, beta2,
                   eps, weight_decay, max_norm, ema_decay, grad_scale, workspace, workspace_bytes, nullptr, nullptr, stream);
}

// ---- the four tails with a learning rate per granule: the sibling's arguments, then lr_group4 and lr_scales in front of the stream
extern "C" int devit_adamw_step_lrs(float* p, const float* g, float* m, float* v, float* ema, void* p_bf16,
                                    const unsigned char* no_decay4, const float* gnorm_sq, const float* dyn, size_t n,
                                    float beta1, float beta2, float eps, float weight_decay, float max_norm, float ema_decay,
                                    float grad_scale, const unsigned char* lr_group4, const float* lr_scales, void* stream) {
  OptArgs a;
  if (int rc = fill_args(a, "devit_adamw_step_lrs", true, p, g, m, v, ema, p_bf16, no_decay4, gnorm_sq, dyn, n, beta1, beta2, eps,
                         weight_decay, max_norm, ema_decay, grad_scale, 0))
    return rc;
  return launch_tail(adamw_lrs_kernel, a, "devit_adamw_step_lrs", lr_group4, lr_scales, stream);
}

extern "C" int devit_sgd_step_lrs(float* p, const float* g, float* buf, float* ema, void* p_bf16, const unsigned char* no_decay4,
                                  const float* gnorm_sq, const float* dyn, size_t n, float momentum, int nesterov,
                                  float weight_decay, float max_norm, float ema_decay, float grad_scale,
                                  const unsigned char* lr_group4, const float* lr_scales, void* stream) {
  OptArgs a;
  if (int rc = fill_args(a, "devit_sgd_step_lrs", false, p, g, buf, nullptr, ema, p_bf16, no_decay4, gnorm_sq, dyn, n, momentum, 0.0f, 0.0f,
                         weight_decay, max_norm, ema_decay, grad_scale, nesterov))
    return rc;
  return launch_tail(sgd_lrs_kernel, a, "devit_sgd_step_lrs", lr_group4, lr_scales, stream);
}

extern "C" int devit_adam_l2_step_lrs(float* p, const float* g, float* m, float* v, float* ema, void* p_bf16,
                                      const unsigned char* no_decay4, const float* gnorm_sq, const float* dyn, size_t n,
                                      float beta1, float beta2, float eps, float weight_decay, float max_norm, float ema_decay,
                                      float grad_scale, const unsigned char* lr_group4, const float* lr_scales, void* stream) {
  OptArgs a;
  if (int rc = fill_args(a, "devit_adam_l2_step_lrs", true, p, g, m, v, ema, p_bf16, no_decay4, gnorm_sq, dyn, n, beta1, beta2, eps,
                         weight_decay, max_norm, ema_decay, grad_scale, 0))
    return rc;
  return launch_tail(adam_l2_lrs_kernel, a, "devit_adam_l2_step_lrs", lr_group4, lr_scales, stream);
}

extern "C" int devit_lamb_step_lrs(float* p, const float* g, float* m, float* v, float* ema, void* p_bf16, const float* gnorm_sq,
                                   const float* dyn, size_t n, const devit_opt_chunk* chunks, int nchunks, int nsegments,
                                   int trust_clip, float beta1, float beta2, float eps, float weight_decay, float max_norm,
                                   float ema_decay, float grad_scale, void* workspace, size_t workspace_bytes,
                                   const unsigned char* lr_group4, const float* lr_scales, void* stream) {
  return lamb_step("devit_lamb_step_lrs", true, p, g, m, v, ema, p_bf16, gnorm_sq, dyn, n, chunks, nchunks, nsegments, trust_clip, beta1,
                   beta2, eps, weight_decay, max_norm, ema_decay, grad_scale, workspace, workspace_bytes, lr_group4, lr_scales, stream);
}
