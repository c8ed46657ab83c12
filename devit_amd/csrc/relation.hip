// The q/k/v feature-relation loss (utils/losses.py:307-328) with both Grams kept on chip: what losses.hip's rel_stats / rel_grad kernels do
// around four batched GEMMs per component, in two launches for all three components.
//   forward  : one workgroup per (image, component).  R_t = F_t F_t^T and R_s = F_s F_s^T accumulate in registers (fp32 MFMA, 64-wide K chunks
//              of the image's rows through LDS; one LDS image serves the A and the B fragments), the row log-sum-exps and KL terms come from
//              the accumulators, the column log-sum-exps cross LDS, and S_unit = coef (P_s + P_s^T - P_t - P_t^T) leaves as bf16.
//   backward : d[:, j Ds : (j + 1) Ds] = bf16(upstream_j * (S_unit F_s)), fp32 accumulation, the device scalar applied in fp32 before the one
//              rounding.  S is read from HBM as the MFMA's B operand, F_s transposed out of LDS (as attention reads V).
// No atomics: every output element has one writer, the loss is finished by a fixed-order reduce.  Rows >= N of an image's window are the next
// image's rows (or pad rows) in the packed buffer: they are never loaded, the LDS image holds zeros there.
#include "gram_pair.h"
#include "reduce.h"

namespace {

struct RelFusedFwdArgs {
  const __bf16* s; const __bf16* t;       // packed qkv buffers (t: bf16 or f16 lanes)
  float* lse_t; float* lse_s; float* row_kl;   // [3][B N]
  __bf16* S;                              // [3][B][208][224]
  int B, N, Ds, Dt, ld_s, ld_t;
  float sc2_t, sc2_s;                     // log2(e) / sqrt(hd): the scaled Grams are held in the base-2 domain
  float coef;                             // 1 / (B sqrt(hd_s))
};

// direct addressing, the diagonal pair only: `img` is the component's first column in the image's head-concatenated rows
#define GP_ACCUM_PARAMS
#define GP_ACCUM_SETUP          \
  constexpr int ci = 0, cj = 0; \
  constexpr bool diag = true;
#define GP_ACCUM_LOAD(dst, u, comp, c)                                                                                      \
  {                                                                                                                         \
    const int sg = tid + u * 512, row = sg >> 3, piece = sg & 7;                                                            \
    dst = (sg < GP_SEGS && row < N) ? *(const bf16x8*)(img + (size_t)row * ld + c * 64 + piece * 8) : zero;                 \
  }
#include "gram_pair_accum.inc"

template <bool TF16>
__global__ __launch_bounds__(512) void rel_fused_fwd_kernel(const RelFusedFwdArgs a) {
  __shared__ __attribute__((aligned(16))) char lds[2 * GP_STAGE];
  __shared__ float lt_sh[GP_ROWS], ls_sh[GP_ROWS];       // base-2 log-sum-exps of the image's rows: the column terms of S
  const int b = blockIdx.x, comp = blockIdx.y, N = a.N;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  const bool two = wave + 8 < GP_TILES;
  const int n = lane & 15, g = lane >> 4;
  f32x4 at[2][GP_TILES], as[2][GP_TILES];
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int J = 0; J < GP_TILES; ++J) at[h][J] = as[h][J] = (f32x4){0.f, 0.f, 0.f, 0.f};
  gram_accumulate<TF16>(a.t + (size_t)b * N * a.ld_t + comp * a.Dt, a.ld_t, a.Dt, N, lds, wave, lane, two, at);
  gram_accumulate<false>(a.s + (size_t)b * N * a.ld_s + comp * a.Ds, a.ld_s, a.Ds, N, lds, wave, lane, two, as);

  const size_t stat0 = (size_t)comp * a.B * N + (size_t)b * N;
#define GP_ONE_ROW 0
#define GP_STATS_SC2_T a.sc2_t
#define GP_STATS_SC2_S a.sc2_s
#define GP_STATS_ADD_TERM(acc, t, s, lt, ls) /* KL: p_t (log p_t - log p_s) */ \
  {                                                                         \
    const float a_t = t - lt, a_s = s - ls;                                 \
    acc += __builtin_amdgcn_exp2f(a_t) * (a_t - a_s);                       \
  }
#define GP_STATS_PUT(i, lt, ls, kl)              \
  {                                              \
    lt_sh[i] = lt;                               \
    ls_sh[i] = ls;                               \
    if (i < N) {                                 \
      a.lse_t[stat0 + i] = lt * (1.0f / LOG2E);  \
      a.lse_s[stat0 + i] = ls * (1.0f / LOG2E);  \
      a.row_kl[stat0 + i] = kl;                  \
    }                                            \
  }
#include "gram_pair_stats.inc"
  __syncthreads();

  // S_unit = coef (P_s + P_s^T - P_t - P_t^T): the Gram is symmetric, the column log-sum-exps ARE the rows' and one slot is written
  __bf16* const Sb = a.S + ((size_t)comp * a.B + b) * GP_ROWS * GP_SLD;
#define GP_EMIT_RLT lt_sh
#define GP_EMIT_RLS ls_sh
#define GP_EMIT_CLT lt_sh
#define GP_EMIT_CLS ls_sh
#define GP_EMIT_COEF a.coef
#define GP_EMIT_ST Sb
#define GP_EMIT_BOTH false
#define GP_EMIT_SR Sb
#define GP_EMIT_LANE lane
#include "gram_pair_emit.inc"
}

struct RelFusedBwdArgs {
  const __bf16* S;          // [3][B][208][224]
  const __bf16* s;          // packed student qkv
  const float* upstream;    // [3] device scalars
  __bf16* d;                // packed gradient, rows < B N written
  int B, N, Ds, ld_s, ld_d;
};
// direct addressing, one product per chunk, the component's own upstream scalar; two workgroups per CU twice over
__global__ __launch_bounds__(512, 4) void rel_fused_bwd_kernel(const RelFusedBwdArgs a) {
  __shared__ __attribute__((aligned(16))) char lds[2 * GP_BSTAGE];
  constexpr int NJ = 1;
  const int b = blockIdx.x, ci = blockIdx.y;
  // the loader's address as a uniform chunk / trip base + one lane offset: row 64 u + tid / 8, piece tid % 8
#define GP_BWD_SETUP                                                          \
  const __bf16* const f = a.s + (size_t)b * N * a.ld_s + ci * a.Ds;           \
  const unsigned foff = (unsigned)(tid >> 3) * (unsigned)a.ld_s + (tid & 7) * 8;
#define GP_BWD_LOAD(dst, u, comp, c)                                                                                          \
  {                                                                                                                           \
    const int row = (tid >> 3) + u * 64;                                                                                      \
    dst = (row < GP_SLD && row < N) ? *(const bf16x8*)((f + c * 64 + (size_t)u * 64 * a.ld_s) + foff) : zero;                 \
  }
// (one product is no loop: a one-trip loop around the prefetch moves instructions of this kernel, which sits at its 128 registers)
#define GP_BWD_EACH_PRODUCT(j) if (constexpr int j = 0; true)
#define GP_BWD_UPSTREAM a.upstream[ci]
#define GP_BWD_OUT(o, i, c) __bf16* const o = a.d + ((size_t)b * N + i) * a.ld_d + ci * a.Ds + c * 64 + 4 * g;
#include "gram_pair_bwd.inc"
}

}  // namespace

extern "C" int devit_relation_fused_fwd(const void* s_qkv, const void* t_qkv, int B, int N, int Ds, int Dt, int ld_s, int ld_t,
                                        int head_dim_t, int head_dim_s, int teacher_f16, float* lse_t, float* lse_s, float* row_kl,
                                        void* S_out, float* loss3, void* stream) {
  DEVIT_CHECK(s_qkv && t_qkv && lse_t && lse_s && row_kl && S_out && loss3, DEVIT_ERR_ARG, "devit_relation_fused_fwd: null pointer");
  DEVIT_CHECK(((uintptr_t)s_qkv | (uintptr_t)t_qkv | (uintptr_t)S_out) % 16 == 0, DEVIT_ERR_ARG,
              "devit_relation_fused_fwd: the qkv buffers and S must be 16-byte aligned");
  DEVIT_CHECK(gram_pair_shape_ok(B, N, Ds, ld_s) && gram_pair_shape_ok(B, N, Dt, ld_t) && head_dim_t > 0 && head_dim_s > 0 &&
                  (long long)B * N < (1ll << 31) / 3,
              DEVIT_ERR_SHAPE,
              "devit_relation_fused_fwd: B=%d N=%d Ds=%d Dt=%d ld_s=%d ld_t=%d: N <= 208, widths multiples of 64 up to 1024, row strides multiples "
              "of 8 and >= 3 widths",
              B, N, Ds, Dt, ld_s, ld_t);
  RelFusedFwdArgs a{(const __bf16*)s_qkv, (const __bf16*)t_qkv, lse_t, lse_s, row_kl, (__bf16*)S_out, B, N, Ds, Dt, ld_s, ld_t,
                    (float)(1.4426950408889634 / sqrt((double)head_dim_t)), (float)(1.4426950408889634 / sqrt((double)head_dim_s)),
                    1.0f / ((float)B * sqrtf((float)head_dim_s))};
  if (teacher_f16) hipLaunchKernelGGL(rel_fused_fwd_kernel<true>, dim3(B, 3), dim3(512), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(rel_fused_fwd_kernel<false>, dim3(B, 3), dim3(512), 0, (hipStream_t)stream, a);
  DEVIT_LAUNCH_CHECK();
  // loss[c] = sum(row_kl[c][:]) / B   (KLDivLoss batchmean), one block per component
  hipLaunchKernelGGL(fixed_order_reduce_kernel, dim3(3), dim3(1024), 0, (hipStream_t)stream, (const float*)row_kl, (long long)B * N, 1.0f / (float)B,
                     loss3);
  DEVIT_LAUNCH_CHECK();
  return DEVIT_OK;
}

extern "C" int devit_relation_fused_bwd(const void* S, const void* s_qkv, const float* upstream3, int B, int N, int Ds, int ld_s, void* d,
                                        int ld_d, void* stream) {
  DEVIT_CHECK(S && s_qkv && upstream3 && d, DEVIT_ERR_ARG, "devit_relation_fused_bwd: null pointer");
  DEVIT_CHECK(((uintptr_t)S | (uintptr_t)s_qkv) % 16 == 0 && (uintptr_t)d % 8 == 0, DEVIT_ERR_ARG,
              "devit_relation_fused_bwd: S and the qkv buffer must be 16-byte aligned, d 8-byte aligned");
  DEVIT_CHECK(gram_pair_shape_ok(B, N, Ds, ld_s) && ld_d >= 3 * Ds && ld_d % 4 == 0, DEVIT_ERR_SHAPE,
              "devit_relation_fused_bwd: B=%d N=%d Ds=%d ld_s=%d ld_d=%d: N <= 208, Ds a multiple of 64 up to 1024, ld_s a multiple of 8, ld_d of 4, "
              "both >= 3 Ds",
              B, N, Ds, ld_s, ld_d);
  RelFusedBwdArgs a{(const __bf16*)S, (const __bf16*)s_qkv, upstream3, (__bf16*)d, B, N, Ds, ld_s, ld_d};
  hipLaunchKernelGGL(rel_fused_bwd_kernel, dim3(B, 3), dim3(512), 0, (hipStream_t)stream, a);
  DEVIT_LAUNCH_CHECK();
  return DEVIT_OK;
}
