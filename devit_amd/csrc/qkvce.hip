// cal_qkv_loss / cal_qkv_loss2 / soft_cross_entropy (utils/losses.py:37-41, 247-292): soft cross-entropies between the row softmaxes of the
// teacher's and the student's pair Grams Z_ij = X_i X_j^T / 8 of the q/k/v components, both Grams kept on chip as csrc/relation.hip keeps its two.
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
#include "devit_common.h"

namespace {

constexpr int QK_ROWS = 208;              // 13 MFMA tiles, as csrc/relation.hip
constexpr int QK_TILES = QK_ROWS / 16;
constexpr int QK_SLD = 224;               // S row stride: seven 32-wide K steps of the backward product
constexpr int QK_STRIDE = 144;            // bytes per LDS row: 64 16-bit elements + 16 bytes
constexpr int QK_STAGE = QK_ROWS * QK_STRIDE;
constexpr int QK_SEGS = QK_ROWS * 8;      // 16-byte pieces of one K chunk

__device__ __forceinline__ float group16_max(float v) {
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ float group16_sum(float v) {
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// over the four 16-lane groups of a wave: the lanes that hold one column
__device__ __forceinline__ float cross4_max(float v) {
  v = fmaxf(v, __shfl_xor(v, 16, 64));
  return fmaxf(v, __shfl_xor(v, 32, 64));
}
__device__ __forceinline__ float cross4_sum(float v) {
  v += __shfl_xor(v, 16, 64);
  return v + __shfl_xor(v, 32, 64);
}

// The chunk map of one model as a table in LDS: entry g = row H + m of (row, 64-wide chunk m) holds token | head << 8, so that the loaders' K loops
// carry one lane value (row0 H) and no division.  view: head g / N, token g % N; tokens: head m, token row.
constexpr int QK_MAP = QK_ROWS * 16;
__device__ __forceinline__ void fill_chunk_map(unsigned* tab, int N, int H, bool view, int tid) {
  for (unsigned e = tid; e < (unsigned)(N * H); e += 512) {
    const unsigned q = e / (unsigned)(view ? N : H), r = e - q * (unsigned)(view ? N : H);
    tab[e] = view ? (r | q << 8) : (q | r << 8);
  }
}
// the offset of the chunk's first element in an image's packed rows (row stride ld, component columns at comp_col)
__device__ __forceinline__ unsigned chunk_off(unsigned entry, int ld, int comp_col) {
  return (entry & 255u) * (unsigned)ld + (entry >> 8) * 64u + (unsigned)comp_col;
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

// acc[h][J] += X_ci[strip h of this wave][:] X_cj[tile J][:]^T over the image's D columns.  Stages 0 / 1 of `lds` hold the A operand's chunks,
// stages 2 / 3 the B operand's (ci != cj).  The A chunk's successor travels through registers under the MFMAs; the B chunk's is fetched behind them
// (one set of prefetch registers beside 2 x 2 x 13 accumulators).  Ends behind a barrier.
template <bool F16>
__device__ __forceinline__ void pair_gram(const __bf16* img, int ld, int D, int N, bool view, int ci, int cj, char* lds, unsigned* tab, int wave,
                                          int lane, bool two, f32x4 (&acc)[2][QK_TILES]) {
  const int tid = threadIdx.x, H = D / 64;
  const bool diag = ci == cj;
  const int row0 = tid >> 3;
  const unsigned row0H = (unsigned)row0 * (unsigned)H;
  const bf16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
  bf16x8 pf[4];
  auto gload = [&](int comp, int c) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int row = row0 + 64 * u;
      pf[u] = (row < QK_ROWS && row < N) ? *(const bf16x8*)(img + (chunk_off(tab[row0H + 64 * u * H + c], ld, comp * D) + (tid & 7) * 8)) : zero;
    }
  };
  auto lstore = [&](int stage) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int sg = tid + u * 512, row = sg >> 3, piece = sg & 7;
      if (sg < QK_SEGS) *(bf16x8*)(lds + stage * QK_STAGE + row * QK_STRIDE + piece * 16) = pf[u];
    }
  };
  fill_chunk_map(tab, N, H, view, tid);
  __syncthreads();
  gload(ci, 0);
  lstore(0);
  if (!diag) {
    gload(cj, 0);
    lstore(2);
  }
  __syncthreads();
  const int frag = (lane & 15) * QK_STRIDE + (lane >> 4) * 16;
  for (int c = 0; c < H; ++c) {
    if (c + 1 < H) gload(ci, c + 1);
    const char* sa = lds + (c & 1) * QK_STAGE + frag;
    const char* sb = diag ? sa : sa + 2 * QK_STAGE;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      const bf16x8 a0 = *(const bf16x8*)(sa + wave * 16 * QK_STRIDE + kk * 64);
      bf16x8 a1 = zero;
      if (two) a1 = *(const bf16x8*)(sa + (wave + 8) * 16 * QK_STRIDE + kk * 64);
#pragma unroll
      for (int J = 0; J < QK_TILES; ++J) {
        const bf16x8 bj = *(const bf16x8*)(sb + J * 16 * QK_STRIDE + kk * 64);
        acc[0][J] = mfma16t<F16>(a0, bj, acc[0][J]);
        if (two) acc[1][J] = mfma16t<F16>(a1, bj, acc[1][J]);
      }
    }
    if (c + 1 < H) {
      lstore((c + 1) & 1);
      if (!diag) {
        gload(cj, c + 1);
        lstore(2 + ((c + 1) & 1));
      }
    }
    __syncthreads();
  }
}

template <bool TF16>
__global__ __launch_bounds__(512) void qkv_pair_fwd_kernel(const QkvFwdArgs a) {
  __shared__ __attribute__((aligned(16))) char lds[4 * QK_STAGE];
  __shared__ unsigned map[QK_MAP];
  const int b = blockIdx.x, N = a.N;
  int ci, cj;
  pair_of(blockIdx.y, ci, cj);
  const bool diag = ci == cj;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  const bool two = wave + 8 < QK_TILES;
  f32x4 at[2][QK_TILES], as[2][QK_TILES];
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int J = 0; J < QK_TILES; ++J) at[h][J] = as[h][J] = (f32x4){0.f, 0.f, 0.f, 0.f};
  pair_gram<TF16>(a.t + (size_t)b * N * a.ld_t, a.ld_t, a.Dt, N, a.view != 0, ci, cj, lds, map, wave, lane, two, at);
  pair_gram<false>(a.s + (size_t)b * N * a.ld_s, a.ld_s, a.Ds, N, a.view != 0, ci, cj, lds, map, wave, lane, two, as);

  // the operand stages are dead (pair_gram ends behind a barrier): the statistics live there.  The lane's coordinates are taken afresh (mbcnt):
  // nothing but the accumulators stays live across the K loops, whose registers are all spoken for
  const int lane_s = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)), tid_s = wave * 64 + lane_s;
  const int n = lane_s & 15, g = lane_s >> 4;
  float* const rlt = (float*)lds;                 // [208] base-2 row log-sum-exps, teacher
  float* const rls = rlt + QK_ROWS;               //       student
  float* const clt = rls + QK_ROWS;               // [208] column log-sum-exps
  float* const cls = clt + QK_ROWS;
  float* const part = cls + QK_ROWS;              // [4][8][208] per-wave column partials
  const size_t BN = (size_t)a.B * N;
  const int slot_ij = a.cross ? 3 * ci + cj : ci, slot_ji = 3 * cj + ci;

  // row statistics: lane (g, n) holds rows 4 g + r of its strips at columns 16 J + n; a row is 13 accumulators x the 16 lanes of a group
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    if (h == 0 || two) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = (wave + 8 * h) * 16 + 4 * g + r;
        float mt = -INFINITY, ms = -INFINITY;
#pragma unroll
        for (int J = 0; J < QK_TILES; ++J) {
          const bool valid = J * 16 + n < N;
          at[h][J][r] = valid ? at[h][J][r] * a.sc2 : -INFINITY;
          as[h][J][r] = valid ? as[h][J][r] * a.sc2 : -INFINITY;
          mt = fmaxf(mt, at[h][J][r]);
          ms = fmaxf(ms, as[h][J][r]);
        }
        mt = group16_max(mt);
        ms = group16_max(ms);
        float st = 0.f, ss = 0.f;
#pragma unroll
        for (int J = 0; J < QK_TILES; ++J) {
          st += __builtin_amdgcn_exp2f(at[h][J][r] - mt);
          ss += __builtin_amdgcn_exp2f(as[h][J][r] - ms);
        }
        const float lt = mt + log2f(group16_sum(st)), ls = ms + log2f(group16_sum(ss));
        float ce = 0.f;
#pragma unroll
        for (int J = 0; J < QK_TILES; ++J)
          if (J * 16 + n < N) ce += __builtin_amdgcn_exp2f(at[h][J][r] - lt) * (ls - as[h][J][r]);
        ce = group16_sum(ce) * (1.0f / LOG2E);
        if (n == 0) {
          rlt[i] = lt;
          rls[i] = ls;
          if (i < N) a.terms[slot_ij * BN + (size_t)b * N + i] = ce;
        }
        __builtin_amdgcn_sched_barrier(0);        // one row at a time: interleaved rows cost registers that 2 x 2 x 13 accumulators leave no room for
      }
    }
  }

  if (!diag) {
    // column log-sum-exps: per wave (max, sum) over its up to 32 rows, combined over the eight waves by the column's thread
#pragma unroll
    for (int J = 0; J < QK_TILES; ++J) {
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
        part[(0 * 8 + wave) * QK_ROWS + j] = mt;
        part[(1 * 8 + wave) * QK_ROWS + j] = st;
        part[(2 * 8 + wave) * QK_ROWS + j] = ms;
        part[(3 * 8 + wave) * QK_ROWS + j] = ss;
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    __syncthreads();
    if (tid_s < QK_ROWS) {
      const int j = tid_s;
      float lt = 0.f, ls = 0.f;
      if (j < N) {
        float mt = -INFINITY, ms = -INFINITY;
#pragma unroll
        for (int w = 0; w < 8; ++w) {
          mt = fmaxf(mt, part[(0 * 8 + w) * QK_ROWS + j]);
          ms = fmaxf(ms, part[(2 * 8 + w) * QK_ROWS + j]);
        }
        float st = 0.f, ss = 0.f;
#pragma unroll
        for (int w = 0; w < 8; ++w) {
          const float pt = part[(0 * 8 + w) * QK_ROWS + j], ps = part[(2 * 8 + w) * QK_ROWS + j];
          st += pt == -INFINITY ? 0.f : part[(1 * 8 + w) * QK_ROWS + j] * __builtin_amdgcn_exp2f(pt - mt);
          ss += ps == -INFINITY ? 0.f : part[(3 * 8 + w) * QK_ROWS + j] * __builtin_amdgcn_exp2f(ps - ms);
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
    for (int J = 0; J < QK_TILES; ++J) {
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
      if (g == 0) part[wave * QK_ROWS + j] = ce;        // (the partials above were consumed before the barrier)
      __builtin_amdgcn_sched_barrier(0);
    }
    __syncthreads();
    if (tid_s < N) {
      const int j = tid_s;
      float ce = 0.f;
#pragma unroll
      for (int w = 0; w < 8; ++w) ce += part[w * QK_ROWS + j];
      a.terms[slot_ji * BN + (size_t)b * N + j] = ce * (1.0f / LOG2E);
    }
  } else {
    __syncthreads();
  }

  // S_ij[i][j] = coef (e^{s - rls_i} + e^{s - cls_j} - e^{t - rlt_i} - e^{t - clt_j}), zero outside N x N; for i == j the column statistics ARE
  // the row statistics.  The lane holds four consecutive i of one column j: one 8-byte store into ROW j of the transposed copy (slot (j, i); for
  // i == j that is the matrix itself), and, for i != j, four 2-byte stores into the rows i of slot (i, j).
  const float* const ct = diag ? rlt : clt;
  const float* const cs = diag ? rls : cls;
  __bf16* const St = a.S + ((size_t)(diag ? slot_ij : slot_ji) * a.B + b) * QK_ROWS * QK_SLD;
  __bf16* const Sr = a.S + ((size_t)slot_ij * a.B + b) * QK_ROWS * QK_SLD;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    if (h == 0 || two) {
      const int i0 = (wave + 8 * h) * 16 + 4 * g;
      float lti[4], lsi[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        lti[r] = rlt[i0 + r];
        lsi[r] = rls[i0 + r];
      }
#pragma unroll
      for (int J = 0; J < QK_TILES; ++J) {
        const int j = J * 16 + n;
        const float ltj = ct[j], lsj = cs[j];
        f32x4 v;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float t = at[h][J][r], s = as[h][J][r];
          const float e = (__builtin_amdgcn_exp2f(s - lsi[r]) + __builtin_amdgcn_exp2f(s - lsj) - __builtin_amdgcn_exp2f(t - lti[r]) -
                           __builtin_amdgcn_exp2f(t - ltj)) * a.coef;
          v[r] = (i0 + r < N && j < N) ? e : 0.f;
        }
        *(bf16x4*)(St + (size_t)j * QK_SLD + i0) = (bf16x4){f2bf(v[0]), f2bf(v[1]), f2bf(v[2]), f2bf(v[3])};
        if (!diag) {
#pragma unroll
          for (int r = 0; r < 4; ++r) Sr[(size_t)(i0 + r) * QK_SLD + j] = f2bf(v[r]);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      // columns 208 .. 223 of the strip's rows: the K tail of the backward product
      const size_t tail = (size_t)((wave + 8 * h) * 16 + (lane_s >> 2)) * QK_SLD + QK_ROWS + (lane_s & 3) * 4;
      *(bf16x4*)(St + tail) = (bf16x4){0, 0, 0, 0};
      if (!diag) *(bf16x4*)(Sr + tail) = (bf16x4){0, 0, 0, 0};
    }
  }
}

// out[0] = scale * sum(src[0 .. n)): one block, rel_fused_reduce_kernel's fixed order
__global__ __launch_bounds__(1024) void qkv_reduce_kernel(const float* src, long long n, float scale, float* out) {
  __shared__ float red[16];
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
    out[0] = t * scale;
  }
}

struct QkvBwdArgs {
  const __bf16* S;          // [P][B][208][224]
  const __bf16* s;          // packed student qkv
  const float* upstream;    // device scalar
  __bf16* d;                // packed gradient, rows < B N written
  int B, N, Ds, ld_s, ld_d, view;
};
// One workgroup per (image, component i): d_i^T[c][r] = sum_j sum_k X_j^T[c][k] S_ij[r][k], 64 columns c at a time, NJ = 1 (j = i) or 3 products per
// chunk.  rel_fused_bwd_kernel's shape: S_ij as the MFMA's B operand from registers (read from HBM once per j), X_j^T by transposed reads from the LDS
// image of the gathered 64-column chunk; the (chunk, j) steps alternate between two stages, the next step's chunk on its way through registers.
constexpr int QB_STAGE = QK_SLD * QK_STRIDE;
constexpr int QB_SEGS = QK_SLD * 8;
template <int NJ>
__global__ __launch_bounds__(512) void qkv_pair_bwd_kernel(const QkvBwdArgs a) {
  __shared__ __attribute__((aligned(16))) char lds[2 * QB_STAGE];
  __shared__ unsigned map[QK_MAP];
  const int b = blockIdx.x, ci = blockIdx.y, N = a.N, H = a.Ds / 64, steps = H * NJ;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63, tid = threadIdx.x;
  const bool two = wave + 8 < QK_TILES, view = a.view != 0;
  const int n = lane & 15, g = lane >> 4;
  const __bf16* const img = a.s + (size_t)b * N * a.ld_s;
  const bf16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
  const unsigned row0H = (unsigned)(tid >> 3) * (unsigned)H;
  bf16x8 pf[4];
  auto gload = [&](int step) {
    const int c = step / NJ, comp = NJ == 1 ? ci : step - c * NJ;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int row = (tid >> 3) + u * 64;
      pf[u] = (row < QK_SLD && row < N)
                  ? *(const bf16x8*)(img + (chunk_off(map[row0H + 64 * u * H + c], a.ld_s, comp * a.Ds) + (tid & 7) * 8)) : zero;
    }
  };
  auto lstore = [&](int stage) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int sg = tid + u * 512, row = sg >> 3, piece = sg & 7;
      if (sg < QB_SEGS) *(bf16x8*)(lds + stage * QB_STAGE + row * QK_STRIDE + piece * 16) = pf[u];
    }
  };
  fill_chunk_map(map, N, H, view, tid);
  __syncthreads();
  gload(0);
  // every element of the slots was written by the forward: all 208 rows x 224 columns are read
  bf16x8 sf[NJ][2][7];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int slot = NJ == 1 ? ci : 3 * ci + j;
    const __bf16* const Sl = a.S + (((size_t)slot * a.B + b) * QK_ROWS + wave * 16 + n) * QK_SLD + g * 8;
#pragma unroll
    for (int ks = 0; ks < 7; ++ks) {
      sf[j][0][ks] = *(const bf16x8*)(Sl + ks * 32);
      sf[j][1][ks] = two ? *(const bf16x8*)(Sl + (size_t)128 * QK_SLD + ks * 32) : zero;
    }
  }
  lstore(0);
  __syncthreads();
  const float up = a.upstream[0];
  const int trd = (8 * g + (n >> 2)) * QK_STRIDE + (n & 3) * 8;
  for (int c = 0; c < H; ++c) {
    f32x4 acc[2][4];
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) acc[h][ct] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int step = c * NJ + j;
      if (step + 1 < steps) gload(step + 1);
      const char* const st = lds + (step & 1) * QB_STAGE + trd;
#pragma unroll
      for (int ks = 0; ks < 7; ++ks) {
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) {
          const char* p = st + ks * 32 * QK_STRIDE + ct * 32;
          const bf16x8 ff = cat8(lds_tr_read(p), lds_tr_read(p + 4 * QK_STRIDE));
          acc[0][ct] = mfma16(ff, sf[j][0][ks], acc[0][ct]);
          if (two) acc[1][ct] = mfma16(ff, sf[j][1][ks], acc[1][ct]);
        }
      }
      if (j == NJ - 1) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int i = (wave + 8 * h) * 16 + n;
          if ((h == 0 || two) && i < N) {
            // the chunk's own place under the layout: row b N + token, columns ci Ds + 64 head ..
            const unsigned off = chunk_off(map[i * H + c], a.ld_d, ci * a.Ds);
            __bf16* const o = a.d + (size_t)b * N * a.ld_d + off + 4 * g;
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) {
              const f32x4 v = acc[h][ct];
              *(bf16x4*)(o + ct * 16) = (bf16x4){f2bf(v[0] * up), f2bf(v[1] * up), f2bf(v[2] * up), f2bf(v[3] * up)};
            }
          }
        }
      }
      if (step + 1 < steps) lstore((step + 1) & 1);
      __syncthreads();
    }
  }
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

bool qkv_pair_shape_ok(int B, int N, int D, int ld) {
  return B > 0 && N > 0 && N <= QK_ROWS && D > 0 && D <= 1024 && D % 64 == 0 && ld >= 3 * D && ld % 8 == 0;
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
  DEVIT_CHECK(qkv_pair_shape_ok(B, N, Ds, ld_s) && qkv_pair_shape_ok(B, N, Dt, ld_t) && (long long)B * N < (1ll << 31) / 9, DEVIT_ERR_SHAPE,
              "devit_qkv_pair_fwd: B=%d N=%d Ds=%d Dt=%d ld_s=%d ld_t=%d: N <= 208, widths multiples of 64 up to 1024, row strides multiples "
              "of 8 and >= 3 widths",
              B, N, Ds, Dt, ld_s, ld_t);
  const int P = cross ? 9 : 3;
  QkvFwdArgs a{(const __bf16*)s_qkv, (const __bf16*)t_qkv, terms, (__bf16*)S_out, B, N, Ds, Dt, ld_s, ld_t, cross, layout == 0,
               (float)(1.4426950408889634 / 8.0), (float)(1.0 / ((double)P * layers * B * N * 8.0))};
  if (teacher_f16) hipLaunchKernelGGL(qkv_pair_fwd_kernel<true>, dim3(B, cross ? 6 : 3), dim3(512), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(qkv_pair_fwd_kernel<false>, dim3(B, cross ? 6 : 3), dim3(512), 0, (hipStream_t)stream, a);
  DEVIT_LAUNCH_CHECK();
  hipLaunchKernelGGL(qkv_reduce_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, (const float*)terms, (long long)P * B * N,
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
  DEVIT_CHECK(qkv_pair_shape_ok(B, N, Ds, ld_s) && ld_d >= 3 * Ds && ld_d % 4 == 0, DEVIT_ERR_SHAPE,
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
  hipLaunchKernelGGL(qkv_reduce_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, (const float*)row_loss, (long long)R, 1.0f / (float)R, loss);
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
