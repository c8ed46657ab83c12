// cal_qkv_loss / cal_qkv_loss2 / soft_cross_entropy (utils/losses.py:37-41, 247-292): soft cross-entropies between the row softmaxes of the
// teacher's and the student's pair Grams Z_ij = X_i X_j^T / 8 of the q/k/v components, both Grams kept on chip: gram_pair.h's tile, shared with
// csrc/relation.hip, under the chunk map.
//   the rows   : the reference's `.contiguous().view(B, N, H * 64)` of a [B, H, N, 64] tensor REINTERPRETS memory.  Row r of the viewed matrix is H
//                chunks of 64 elements; with g = r H + m, chunk m is the head vector of head g / N and token g % N -- in the packed qkv buffer row
//                b N + g % N, columns comp D + 64 (g / N) .. + 63.  A bijection on the 64-wide chunks of an image: the loaders gather by it, the
//                backward scatters by it with one writer per chunk.  layout 1 ("tokens") is the identity map, head-concatenated rows.
//   forward    : one workgroup per (image, unordered pair): (i, i) for the self mode, plus (0, 1), (0, 2), (1, 2) for the cross mode.  The A and B
//                operands are two LDS images (one when i == j); the ordered pair (j, i) is the same Gram with the softmax over columns, so the
//                column log-sum-exps and column terms cross LDS (a column spans all eight waves' strips), in a fixed order.
//                S_ij = coef (dP_rows + dP_cols), dP = softmax(Z_s) - softmax(Z_t), leaves as bf16 [208][224] in the slot (i, j) of the backward's
//                `sum_j S_ij X_j`; the forward ALSO stores the transposed copy S_ji = S_ij^T into the slot (j, i) (the backward never reads
//                transposed).  For i == j the two coincide (S_ii is symmetric) and one slot is written.
//   backward   : one workgroup per (image, component i): d_i = bf16(upstream * sum_j S_ij X_j), fp32 accumulation over the one (self) or three
//                (cross) products, the device scalar applied in fp32 before the one rounding; X_j gathered, d_i scattered through the chunk map.
//   soft_ce    : soft_cross_entropy on fp32 rows [R, C], one wave per row.
// No atomics: every output element has one writer and every sum a fixed order.  Rows >= N of an image are never loaded (zeros in LDS).
#include "gram_pair.h"
#include "reduce.h"

namespace {

// over the four 16-lane groups of a wave: the lanes that hold one column
__device__ __forceinline__ float cross4_max(float v) {
  v = fmaxf(v, __shfl_xor(v, 16, 64));
  return fmaxf(v, __shfl_xor(v, 32, 64));
}
__device__ __forceinline__ float cross4_sum(float v) {
  v += __shfl_xor(v, 16, 64);
  return v + __shfl_xor(v, 32, 64);
}

// the unordered pair p: 0 .. 2 are (p, p), 3 .. 5 are (0, 1), (0, 2), (1, 2)
__device__ __forceinline__ void pair_of(int p, int& i, int& j) {
  i = p < 3 ? p : (p == 5 ? 1 : 0);
  j = p < 3 ? p : (p == 3 ? 1 : 2);
}

struct QkvFwdArgs {
  const __bf16* s; const __bf16* t;       // packed qkv buffers (t: bf16 or f16 lanes)
  float* terms;                           // [P][B N] row terms of the ordered pairs, P = 3 (slot i) or 9 (slot 3 i + j)
  __bf16* S;                              // [P][B][208][224]
  int B, N, Ds, Dt, ld_s, ld_t, cross, view;
  float sc2;                              // log2(e) / 8: the scaled Grams are held in the base-2 domain
  float coef;                             // 1 / (P layers B N 8)
};

// chunk-map addressing, any pair: `img` is the image's first packed row, the table is rebuilt per call (the two models differ in H)
#define GP_ACCUM_PARAMS bool view, int ci, int cj, unsigned* tab,
#define GP_ACCUM_SETUP                                        \
  const bool diag = ci == cj;                                 \
  const int row0 = tid >> 3;                                  \
  const unsigned row0H = (unsigned)row0 * (unsigned)nch;      \
  fill_chunk_map(tab, N, nch, view, tid);                     \
  __syncthreads();
#define GP_ACCUM_LOAD(dst, u, comp, c)                                                                                                        \
  {                                                                                                                                           \
    const int row = row0 + 64 * u;                                                                                                            \
    dst = (row < GP_ROWS && row < N) ? *(const bf16x8*)GP_CHUNK_MAP_PIECE(img, tab, row0H, nch, u, c, ld, comp * D) : zero;                     \
  }
#include "gram_pair_accum.inc"

template <bool TF16>
__global__ __launch_bounds__(512) void qkv_pair_fwd_kernel(const QkvFwdArgs a) {
  __shared__ __attribute__((aligned(16))) char lds[4 * GP_STAGE];
  __shared__ unsigned map[GP_MAP];
  const int b = blockIdx.x, N = a.N;
  int ci, cj;
  pair_of(blockIdx.y, ci, cj);
  const bool diag = ci == cj;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  const bool two = wave + 8 < GP_TILES;
  f32x4 at[2][GP_TILES], as[2][GP_TILES];
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int J = 0; J < GP_TILES; ++J) at[h][J] = as[h][J] = (f32x4){0.f, 0.f, 0.f, 0.f};
  gram_accumulate<TF16>(a.t + (size_t)b * N * a.ld_t, a.ld_t, a.Dt, N, a.view != 0, ci, cj, map, lds, wave, lane, two, at);
  gram_accumulate<false>(a.s + (size_t)b * N * a.ld_s, a.ld_s, a.Ds, N, a.view != 0, ci, cj, map, lds, wave, lane, two, as);

  // the operand stages are dead (gram_accumulate ends behind a barrier): the statistics live there.  The lane's coordinates are taken afresh (mbcnt):
  // nothing but the accumulators stays live across the K loops, whose registers are all spoken for
  const int lane_s = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)), tid_s = wave * 64 + lane_s;
  const int n = lane_s & 15, g = lane_s >> 4;
  float* const rlt = (float*)lds;                 // [208] base-2 row log-sum-exps, teacher
  float* const rls = rlt + GP_ROWS;               //       student
  float* const clt = rls + GP_ROWS;               // [208] column log-sum-exps
  float* const cls = clt + GP_ROWS;
  float* const part = cls + GP_ROWS;              // [4][8][208] per-wave column partials
  const size_t BN = (size_t)a.B * N;
  const int slot_ij = a.cross ? 3 * ci + cj : ci, slot_ji = 3 * cj + ci;

#define GP_ONE_ROW 1
#define GP_STATS_SC2_T a.sc2
#define GP_STATS_SC2_S a.sc2
#define GP_STATS_ADD_TERM(acc, t, s, lt, ls) acc += __builtin_amdgcn_exp2f(t - lt) * (ls - s);       /* CE: -p_t log p_s */
#define GP_STATS_PUT(i, lt, ls, ce)                                  \
  {                                                                  \
    rlt[i] = lt;                                                     \
    rls[i] = ls;                                                     \
    if (i < N) a.terms[slot_ij * BN + (size_t)b * N + i] = ce;       \
  }
#include "gram_pair_stats.inc"

  if (!diag) {
    // column log-sum-exps: per wave (max, sum) over its up to 32 rows, combined over the eight waves by the column's thread
#pragma unroll
    for (int J = 0; J < GP_TILES; ++J) {
      float mt = -INFINITY, ms = -INFINITY;
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const bool live = (h == 0 || two) && (wave + 8 * h) * 16 + 4 * g + r < N;
          mt = fmaxf(mt, live ? at[h][J][r] : -INFINITY);
          ms = fmaxf(ms, live ? as[h][J][r] : -INFINITY);
        }
      mt = cross4_max(mt);
      ms = cross4_max(ms);
      const float bt = mt == -INFINITY ? 0.f : mt, bs = ms == -INFINITY ? 0.f : ms;
      float st = 0.f, ss = 0.f;
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const bool live = (h == 0 || two) && (wave + 8 * h) * 16 + 4 * g + r < N;
          st += live ? __builtin_amdgcn_exp2f(at[h][J][r] - bt) : 0.f;
          ss += live ? __builtin_amdgcn_exp2f(as[h][J][r] - bs) : 0.f;
        }
      st = cross4_sum(st);
      ss = cross4_sum(ss);
      if (g == 0) {
        const int j = J * 16 + n;
        part[(0 * 8 + wave) * GP_ROWS + j] = mt;
        part[(1 * 8 + wave) * GP_ROWS + j] = st;
        part[(2 * 8 + wave) * GP_ROWS + j] = ms;
        part[(3 * 8 + wave) * GP_ROWS + j] = ss;
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    __syncthreads();
    if (tid_s < GP_ROWS) {
      const int j = tid_s;
      float lt = 0.f, ls = 0.f;
      if (j < N) {
        float mt = -INFINITY, ms = -INFINITY;
#pragma unroll
        for (int w = 0; w < 8; ++w) {
          mt = fmaxf(mt, part[(0 * 8 + w) * GP_ROWS + j]);
          ms = fmaxf(ms, part[(2 * 8 + w) * GP_ROWS + j]);
        }
        float st = 0.f, ss = 0.f;
#pragma unroll
        for (int w = 0; w < 8; ++w) {
          const float pt = part[(0 * 8 + w) * GP_ROWS + j], ps = part[(2 * 8 + w) * GP_ROWS + j];
          st += pt == -INFINITY ? 0.f : part[(1 * 8 + w) * GP_ROWS + j] * __builtin_amdgcn_exp2f(pt - mt);
          ss += ps == -INFINITY ? 0.f : part[(3 * 8 + w) * GP_ROWS + j] * __builtin_amdgcn_exp2f(ps - ms);
        }
        lt = mt + log2f(st);
        ls = ms + log2f(ss);
      }
      clt[j] = lt;
      cls[j] = ls;
    }
    __syncthreads();
    // column terms of the ordered pair (j, i): sum_i softmax_col(Z_t)_ij (ls_j - Z_s_ij)
#pragma unroll
    for (int J = 0; J < GP_TILES; ++J) {
      const int j = J * 16 + n;
      const float lt = clt[j], ls = cls[j];
      float ce = 0.f;
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const bool live = (h == 0 || two) && (wave + 8 * h) * 16 + 4 * g + r < N && j < N;
          ce += live ? __builtin_amdgcn_exp2f(at[h][J][r] - lt) * (ls - as[h][J][r]) : 0.f;
        }
      ce = cross4_sum(ce);
      if (g == 0) part[wave * GP_ROWS + j] = ce;        // (the partials above were consumed before the barrier)
      __builtin_amdgcn_sched_barrier(0);
    }
    __syncthreads();
    if (tid_s < N) {
      const int j = tid_s;
      float ce = 0.f;
#pragma unroll
      for (int w = 0; w < 8; ++w) ce += part[w * GP_ROWS + j];
      a.terms[slot_ji * BN + (size_t)b * N + j] = ce * (1.0f / LOG2E);
    }
  } else {
    __syncthreads();
  }

  // S_ij = coef (dP_rows + dP_cols); for i == j the column statistics ARE the row statistics.  The 8-byte stores go to the transposed copy, slot
  // (j, i) (for i == j that is the matrix itself); for i != j the per-element stores fill slot (i, j).
  const float* const ct = diag ? rlt : clt;
  const float* const cs = diag ? rls : cls;
  __bf16* const St = a.S + ((size_t)(diag ? slot_ij : slot_ji) * a.B + b) * GP_ROWS * GP_SLD;
  __bf16* const Sr = a.S + ((size_t)slot_ij * a.B + b) * GP_ROWS * GP_SLD;
#define GP_EMIT_RLT rlt
#define GP_EMIT_RLS rls
#define GP_EMIT_CLT ct
#define GP_EMIT_CLS cs
#define GP_EMIT_COEF a.coef
#define GP_EMIT_ST St
#define GP_EMIT_BOTH !diag
#define GP_EMIT_SR Sr
#define GP_EMIT_LANE lane_s
#include "gram_pair_emit.inc"
}

struct QkvBwdArgs {
  const __bf16* S;          // [P][B][208][224]
  const __bf16* s;          // packed student qkv
  const float* upstream;    // device scalar
  __bf16* d;                // packed gradient, rows < B N written
  int B, N, Ds, ld_s, ld_d, view;
};
// chunk-map addressing (X_j gathered, d_i scattered through the table, one writer per chunk), NJ = 1 (self) or 3 (cross) products per chunk
template <int NJ>
__global__ __launch_bounds__(512) void qkv_pair_bwd_kernel(const QkvBwdArgs a) {
  __shared__ __attribute__((aligned(16))) char lds[2 * GP_BSTAGE];
  __shared__ unsigned map[GP_MAP];
  const int b = blockIdx.x, ci = blockIdx.y;
  const bool view = a.view != 0;
#define GP_BWD_SETUP                                              \
  const __bf16* const img = a.s + (size_t)b * N * a.ld_s;         \
  const unsigned row0H = (unsigned)(tid >> 3) * (unsigned)nch;    \
  fill_chunk_map(map, N, nch, view, tid);                         \
  __syncthreads();
#define GP_BWD_LOAD(dst, u, comp, c)                                                                                                   \
  {                                                                                                                                    \
    const int row = (tid >> 3) + u * 64;                                                                                               \
    dst = (row < GP_SLD && row < N) ? *(const bf16x8*)GP_CHUNK_MAP_PIECE(img, map, row0H, nch, u, c, a.ld_s, comp * a.Ds) : zero;      \
  }
#define GP_BWD_EACH_PRODUCT(j) _Pragma("unroll") for (int j = 0; j < NJ; ++j)
#define GP_BWD_UPSTREAM a.upstream[0]
#define GP_BWD_OUT(o, i, c)                                                      \
  const unsigned off = chunk_off(map[i * nch + c], a.ld_d, ci * a.Ds);           \
  __bf16* const o = a.d + (size_t)b * N * a.ld_d + off + 4 * g;
#include "gram_pair_bwd.inc"
}

// ---- soft_cross_entropy on fp32 rows: one wave per row, strided over the C columns -------------------------------------------------------
// x log2(e), rounded as a product of its own (never contracted into the subtraction behind it: a one-column row is then exactly 0)
__device__ __forceinline__ float to2(float x) {
#pragma clang fp contract(off)
  return x * LOG2E;
}
__device__ __forceinline__ void row_lse2(const float* x, int C, int lane, float& m, float& l) {     // base-2 max and log-sum-exp of x log2(e)
  m = -INFINITY;
  for (int j = lane; j < C; j += 64) m = fmaxf(m, to2(x[j]));
  m = wave_max(m);
  float s = 0.f;
  for (int j = lane; j < C; j += 64) s += __builtin_amdgcn_exp2f(to2(x[j]) - m);
  l = m + log2f(wave_sum(s));
}
__global__ __launch_bounds__(256) void soft_ce_rows_fwd_kernel(const float* p, const float* t, int R, int C, float* row_loss) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= R) return;
  const float* pr = p + (size_t)row * C;
  const float* tr = t + (size_t)row * C;
  float mp, lp, mt, lt;
  row_lse2(pr, C, lane, mp, lp);
  row_lse2(tr, C, lane, mt, lt);
  float ce = 0.f;
  for (int j = lane; j < C; j += 64) ce += __builtin_amdgcn_exp2f(to2(tr[j]) - lt) * (lp - to2(pr[j]));
  ce = wave_sum(ce);
  if (lane == 0) row_loss[row] = ce * (1.0f / LOG2E);
}
__global__ __launch_bounds__(256) void soft_ce_rows_bwd_kernel(const float* p, const float* t, const float* upstream, int R, int C, float* dp) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= R) return;
  const float* pr = p + (size_t)row * C;
  const float* tr = t + (size_t)row * C;
  float mp, lp, mt, lt;
  row_lse2(pr, C, lane, mp, lp);
  row_lse2(tr, C, lane, mt, lt);
  const float sc = upstream[0] / (float)R;
  for (int j = lane; j < C; j += 64)
    dp[(size_t)row * C + j] = (__builtin_amdgcn_exp2f(to2(pr[j]) - lp) - __builtin_amdgcn_exp2f(to2(tr[j]) - lt)) * sc;
}

}  // namespace

extern "C" int devit_qkv_pair_fwd(const void* s_qkv, const void* t_qkv, int B, int N, int Ds, int Dt, int ld_s, int ld_t, int head_dim_s,
                                  int head_dim_t, int teacher_f16, int cross, int layout, int layers, float* terms, void* S_out, float* loss,
                                  void* stream) {
  DEVIT_CHECK(s_qkv && t_qkv && terms && S_out && loss, DEVIT_ERR_ARG, "devit_qkv_pair_fwd: null pointer");
  DEVIT_CHECK(((uintptr_t)s_qkv | (uintptr_t)t_qkv | (uintptr_t)S_out) % 16 == 0, DEVIT_ERR_ARG,
              "devit_qkv_pair_fwd: the qkv buffers and S must be 16-byte aligned");
  DEVIT_CHECK((cross == 0 || cross == 1) && (layout == 0 || layout == 1) && layers > 0, DEVIT_ERR_ARG,
              "devit_qkv_pair_fwd: cross=%d layout=%d layers=%d: cross 0 (self) or 1, layout 0 (view) or 1 (tokens), layers > 0", cross, layout,
              layers);
  DEVIT_CHECK(head_dim_s == 64 && head_dim_t == 64, DEVIT_ERR_SHAPE,
              "devit_qkv_pair_fwd: head_dim_s=%d head_dim_t=%d: the chunk map is built on 64-wide heads", head_dim_s, head_dim_t);
  DEVIT_CHECK(gram_pair_shape_ok(B, N, Ds, ld_s) && gram_pair_shape_ok(B, N, Dt, ld_t) && (long long)B * N < (1ll << 31) / 9, DEVIT_ERR_SHAPE,
              "devit_qkv_pair_fwd: B=%d N=%d Ds=%d Dt=%d ld_s=%d ld_t=%d: N <= 208, widths multiples of 64 up to 1024, row strides multiples "
              "of 8 and >= 3 widths",
              B, N, Ds, Dt, ld_s, ld_t);
  const int P = cross ? 9 : 3;
  QkvFwdArgs a{(const __bf16*)s_qkv, (const __bf16*)t_qkv, terms, (__bf16*)S_out, B, N, Ds, Dt, ld_s, ld_t, cross, layout == 0,
               (float)(1.4426950408889634 / 8.0), (float)(1.0 / ((double)P * layers * B * N * 8.0))};
  if (teacher_f16) hipLaunchKernelGGL(qkv_pair_fwd_kernel<true>, dim3(B, cross ? 6 : 3), dim3(512), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(qkv_pair_fwd_kernel<false>, dim3(B, cross ? 6 : 3), dim3(512), 0, (hipStream_t)stream, a);
  DEVIT_LAUNCH_CHECK();
  hipLaunchKernelGGL(fixed_order_reduce_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, (const float*)terms, (long long)P * B * N,
                     (float)(1.0 / ((double)P * layers * B * N)), loss);
  DEVIT_LAUNCH_CHECK();
  return DEVIT_OK;
}

extern "C" int devit_qkv_pair_bwd(const void* S, const void* s_qkv, const float* upstream, int B, int N, int Ds, int ld_s, int head_dim_s,
                                  int cross, int layout, void* d, int ld_d, void* stream) {
  DEVIT_CHECK(S && s_qkv && upstream && d, DEVIT_ERR_ARG, "devit_qkv_pair_bwd: null pointer");
  DEVIT_CHECK(((uintptr_t)S | (uintptr_t)s_qkv) % 16 == 0 && (uintptr_t)d % 8 == 0, DEVIT_ERR_ARG,
              "devit_qkv_pair_bwd: S and the qkv buffer must be 16-byte aligned, d 8-byte aligned");
  DEVIT_CHECK((cross == 0 || cross == 1) && (layout == 0 || layout == 1), DEVIT_ERR_ARG,
              "devit_qkv_pair_bwd: cross=%d layout=%d: cross 0 (self) or 1, layout 0 (view) or 1 (tokens)", cross, layout);
  DEVIT_CHECK(head_dim_s == 64, DEVIT_ERR_SHAPE, "devit_qkv_pair_bwd: head_dim_s=%d: the chunk map is built on 64-wide heads", head_dim_s);
  DEVIT_CHECK(gram_pair_shape_ok(B, N, Ds, ld_s) && ld_d >= 3 * Ds && ld_d % 4 == 0, DEVIT_ERR_SHAPE,
              "devit_qkv_pair_bwd: B=%d N=%d Ds=%d ld_s=%d ld_d=%d: N <= 208, Ds a multiple of 64 up to 1024, ld_s a multiple of 8, ld_d of 4, "
              "both >= 3 Ds",
              B, N, Ds, ld_s, ld_d);
  QkvBwdArgs a{(const __bf16*)S, (const __bf16*)s_qkv, upstream, (__bf16*)d, B, N, Ds, ld_s, ld_d, layout == 0};
  if (cross) hipLaunchKernelGGL(qkv_pair_bwd_kernel<3>, dim3(B, 3), dim3(512), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(qkv_pair_bwd_kernel<1>, dim3(B, 3), dim3(512), 0, (hipStream_t)stream, a);
  DEVIT_LAUNCH_CHECK();
  return DEVIT_OK;
}

extern "C" int devit_soft_ce_rows_fwd(const float* predicts, const float* targets, int R, int C, float* row_loss, float* loss, void* stream) {
  DEVIT_CHECK(predicts && targets && row_loss && loss, DEVIT_ERR_ARG, "devit_soft_ce_rows_fwd: null pointer");
  DEVIT_CHECK(R > 0 && C > 0, DEVIT_ERR_SHAPE, "devit_soft_ce_rows_fwd: R=%d C=%d: both must be >= 1", R, C);
  hipLaunchKernelGGL(soft_ce_rows_fwd_kernel, dim3((R + 3) / 4), dim3(256), 0, (hipStream_t)stream, predicts, targets, R, C, row_loss);
  DEVIT_LAUNCH_CHECK();
  hipLaunchKernelGGL(fixed_order_reduce_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, (const float*)row_loss, (long long)R, 1.0f / (float)R, loss);
  DEVIT_LAUNCH_CHECK();
  return DEVIT_OK;
}

extern "C" int devit_soft_ce_rows_bwd(const float* predicts, const float* targets, const float* upstream, int R, int C, float* d_predicts,
                                      void* stream) {
  DEVIT_CHECK(predicts && targets && upstream && d_predicts, DEVIT_ERR_ARG, "devit_soft_ce_rows_bwd: null pointer");
  DEVIT_CHECK(R > 0 && C > 0, DEVIT_ERR_SHAPE, "devit_soft_ce_rows_bwd: R=%d C=%d: both must be >= 1", R, C);
  hipLaunchKernelGGL(soft_ce_rows_bwd_kernel, dim3((R + 3) / 4), dim3(256), 0, (hipStream_t)stream, predicts, targets, upstream, R, C, d_predicts);
  DEVIT_LAUNCH_CHECK();
  return DEVIT_OK;
}
