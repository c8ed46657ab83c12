// The q/k/v feature-relation loss (utils/losses.py:307-328) with both Grams kept on chip: what losses.hip's rel_stats / rel_grad kernels do
// around four batched GEMMs per component, in two launches for all three components.
//   forward  : one workgroup per (image, component).  R_t = F_t F_t^T and R_s = F_s F_s^T accumulate in registers (fp32 MFMA, 64-wide K chunks
//              of the image's rows through LDS; one LDS image serves the A and the B fragments), the row log-sum-exps and KL terms come from
//              the accumulators, the column log-sum-exps cross LDS, and S_unit = coef (P_s + P_s^T - P_t - P_t^T) leaves as bf16.
//   backward : d[:, j Ds : (j + 1) Ds] = bf16(upstream_j * (S_unit F_s)), fp32 accumulation, the device scalar applied in fp32 before the one
//              rounding.  S is read from HBM as the MFMA's B operand, F_s transposed out of LDS (as attention reads V).
// No atomics: every output element has one writer, the loss is finished by a fixed-order reduce.  Rows >= N of an image's window are the next
// image's rows (or pad rows) in the packed buffer: they are never loaded, the LDS image holds zeros there.
#include "devit_common.h"

namespace {

constexpr int RF_ROWS = 208;              // 13 MFMA tiles: the attention kernels' row limit
constexpr int RF_TILES = RF_ROWS / 16;
constexpr int RF_SLD = 224;               // S row stride: seven 32-wide K steps of the backward product
constexpr int RF_STRIDE = 144;            // bytes per LDS row: 64 16-bit elements + 16 bytes, so that 16 rows' 16-byte reads spread over the banks
constexpr int RF_STAGE = RF_ROWS * RF_STRIDE;
constexpr int RF_SEGS = RF_ROWS * 8;      // 16-byte pieces of one K chunk

struct RelFusedFwdArgs {
  const __bf16* s; const __bf16* t;       // packed qkv buffers (t: bf16 or f16 lanes)
  float* lse_t; float* lse_s; float* row_kl;   // [3][B N]
  __bf16* S;                              // [3][B][208][224]
  int B, N, Ds, Dt, ld_s, ld_t;
  float sc2_t, sc2_s;                     // log2(e) / sqrt(hd): the scaled Grams are held in the base-2 domain
  float coef;                             // 1 / (B sqrt(hd_s))
};

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

// acc[h][J] += F[strip h of this wave][:] F[tile J][:]^T over the D columns at f (row stride ld, N live rows).  Wave w owns the 16-row strips
// w and w + 8 (`two`: the second exists); every strip spans all 13 column tiles, so a row's statistics stay inside one wave.
// Ends behind a barrier: the stages may be rewritten at once.
template <bool F16>
__device__ __forceinline__ void gram_accumulate(const __bf16* f, int ld, int D, int N, char* lds, int wave, int lane, bool two,
                                                f32x4 (&acc)[2][RF_TILES]) {
  const int tid = threadIdx.x;
  const bf16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
  bf16x8 pf[4];
  auto gload = [&](int c) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int sg = tid + u * 512, row = sg >> 3, piece = sg & 7;
      pf[u] = (sg < RF_SEGS && row < N) ? *(const bf16x8*)(f + (size_t)row * ld + c * 64 + piece * 8) : zero;
    }
  };
  auto lstore = [&](int stage) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int sg = tid + u * 512, row = sg >> 3, piece = sg & 7;
      if (sg < RF_SEGS) *(bf16x8*)(lds + stage * RF_STAGE + row * RF_STRIDE + piece * 16) = pf[u];
    }
  };
  const int nch = D / 64;
  gload(0);
  lstore(0);
  __syncthreads();
  const int frag = (lane & 15) * RF_STRIDE + (lane >> 4) * 16;     // row x of a tile, k = 8 g .. 8 g + 7 of a 32-wide step
  for (int c = 0; c < nch; ++c) {
    if (c + 1 < nch) gload(c + 1);
    const char* st = lds + (c & 1) * RF_STAGE + frag;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      const bf16x8 a0 = *(const bf16x8*)(st + wave * 16 * RF_STRIDE + kk * 64);
      bf16x8 a1 = zero;
      if (two) a1 = *(const bf16x8*)(st + (wave + 8) * 16 * RF_STRIDE + kk * 64);
#pragma unroll
      for (int J = 0; J < RF_TILES; ++J) {
        const bf16x8 bj = *(const bf16x8*)(st + J * 16 * RF_STRIDE + kk * 64);
        acc[0][J] = mfma16t<F16>(a0, bj, acc[0][J]);
        if (two) acc[1][J] = mfma16t<F16>(a1, bj, acc[1][J]);
      }
    }
    if (c + 1 < nch) lstore((c + 1) & 1);
    __syncthreads();
  }
}

template <bool TF16>
__global__ __launch_bounds__(512) void rel_fused_fwd_kernel(const RelFusedFwdArgs a) {
  __shared__ __attribute__((aligned(16))) char lds[2 * RF_STAGE];
  __shared__ float lt_sh[RF_ROWS], ls_sh[RF_ROWS];       // base-2 log-sum-exps of the image's rows: the column terms of S
  const int b = blockIdx.x, comp = blockIdx.y, N = a.N;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  const bool two = wave + 8 < RF_TILES;
  const int n = lane & 15, g = lane >> 4;
  f32x4 at[2][RF_TILES], as[2][RF_TILES];
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int J = 0; J < RF_TILES; ++J) at[h][J] = as[h][J] = (f32x4){0.f, 0.f, 0.f, 0.f};
  gram_accumulate<TF16>(a.t + (size_t)b * N * a.ld_t + comp * a.Dt, a.ld_t, a.Dt, N, lds, wave, lane, two, at);
  gram_accumulate<false>(a.s + (size_t)b * N * a.ld_s + comp * a.Ds, a.ld_s, a.Ds, N, lds, wave, lane, two, as);

  // row statistics: lane (g, n) holds rows 4 g + r of its strips at columns 16 J + n; a row is 13 accumulators x the 16 lanes of a group
  const size_t stat0 = (size_t)comp * a.B * N + (size_t)b * N;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    if (h == 0 || two) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = (wave + 8 * h) * 16 + 4 * g + r;
        float mt = -INFINITY, ms = -INFINITY;
#pragma unroll
        for (int J = 0; J < RF_TILES; ++J) {
          const bool valid = J * 16 + n < N;
          at[h][J][r] = valid ? at[h][J][r] * a.sc2_t : -INFINITY;
          as[h][J][r] = valid ? as[h][J][r] * a.sc2_s : -INFINITY;
          mt = fmaxf(mt, at[h][J][r]);
          ms = fmaxf(ms, as[h][J][r]);
        }
        mt = group16_max(mt);
        ms = group16_max(ms);
        float st = 0.f, ss = 0.f;
#pragma unroll
        for (int J = 0; J < RF_TILES; ++J) {
          st += __builtin_amdgcn_exp2f(at[h][J][r] - mt);
          ss += __builtin_amdgcn_exp2f(as[h][J][r] - ms);
        }
        const float lt = mt + log2f(group16_sum(st)), ls = ms + log2f(group16_sum(ss));
        float kl = 0.f;
#pragma unroll
        for (int J = 0; J < RF_TILES; ++J)
          if (J * 16 + n < N) {
            const float a_t = at[h][J][r] - lt, a_s = as[h][J][r] - ls;
            kl += __builtin_amdgcn_exp2f(a_t) * (a_t - a_s);
          }
        kl = group16_sum(kl) * (1.0f / LOG2E);
        if (n == 0) {
          lt_sh[i] = lt;
          ls_sh[i] = ls;
          if (i < N) {
            a.lse_t[stat0 + i] = lt * (1.0f / LOG2E);
            a.lse_s[stat0 + i] = ls * (1.0f / LOG2E);
            a.row_kl[stat0 + i] = kl;
          }
        }
      }
    }
  }
  __syncthreads();

  // S_unit[i][j] = coef (e^{s - ls_i} + e^{s - ls_j} - e^{t - lt_i} - e^{t - lt_j}), zero outside N x N.  The lane holds four consecutive i of one
  // column j: it writes them as one 8-byte store into ROW j (S is symmetric; the value computed at (i, j) is as good a rounding of S_ji).
  __bf16* const Sb = a.S + ((size_t)comp * a.B + b) * RF_ROWS * RF_SLD;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    if (h == 0 || two) {
      const int i0 = (wave + 8 * h) * 16 + 4 * g;
      float lti[4], lsi[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        lti[r] = lt_sh[i0 + r];
        lsi[r] = ls_sh[i0 + r];
      }
#pragma unroll
      for (int J = 0; J < RF_TILES; ++J) {
        const int j = J * 16 + n;
        const float ltj = lt_sh[j], lsj = ls_sh[j];
        f32x4 v;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float t = at[h][J][r], s = as[h][J][r];
          const float e = (__builtin_amdgcn_exp2f(s - lsi[r]) + __builtin_amdgcn_exp2f(s - lsj) - __builtin_amdgcn_exp2f(t - lti[r]) -
                           __builtin_amdgcn_exp2f(t - ltj)) * a.coef;
          v[r] = (i0 + r < N && j < N) ? e : 0.f;
        }
        *(bf16x4*)(Sb + (size_t)j * RF_SLD + i0) = (bf16x4){f2bf(v[0]), f2bf(v[1]), f2bf(v[2]), f2bf(v[3])};
      }
      // columns 208 .. 223 of the strip's rows: the K tail of the backward product
      *(bf16x4*)(Sb + (size_t)((wave + 8 * h) * 16 + (lane >> 2)) * RF_SLD + RF_ROWS + (lane & 3) * 4) = (bf16x4){0, 0, 0, 0};
    }
  }
}

// loss[c] = sum(row_kl[c][:]) / B   (KLDivLoss batchmean): rel_reduce_kernel's fixed order, one block per component
__global__ __launch_bounds__(1024) void rel_fused_reduce_kernel(const float* row_kl, int n, float inv_b, float* loss) {
  __shared__ float red[16];
  const float* src = row_kl + (size_t)blockIdx.x * n;
  float p[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int i0 = threadIdx.x; i0 < n; i0 += 8 * 1024) {
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int i = i0 + u * 1024;
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
    loss[blockIdx.x] = t * inv_b;
  }
}

struct RelFusedBwdArgs {
  const __bf16* S;          // [3][B][208][224]
  const __bf16* s;          // packed student qkv
  const float* upstream;    // [3] device scalars
  __bf16* d;                // packed gradient, rows < B N written
  int B, N, Ds, ld_s, ld_d;
};
// One workgroup per (image, component): d^T[c][i] = sum_k F^T[c][k] S[i][k], 64 columns c at a time.  B = the image's S, read from HBM once into
// registers (lane (n, g): row 16 it + n, k = 32 ks + 8 g .. + 7; wave w owns the row tiles w and w + 8); A = F^T by transposed reads from the LDS
// image of the 64-column chunk, whose successor is on its way through registers meanwhile (as the forward's K chunks).
constexpr int RB_STAGE = RF_SLD * RF_STRIDE;
constexpr int RB_SEGS = RF_SLD * 8;
__global__ __launch_bounds__(512, 4) void rel_fused_bwd_kernel(const RelFusedBwdArgs a) {
  __shared__ __attribute__((aligned(16))) char lds[2 * RB_STAGE];
  const int b = blockIdx.x, comp = blockIdx.y, N = a.N, nch = a.Ds / 64;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63, tid = threadIdx.x;
  const bool two = wave + 8 < RF_TILES;
  const int n = lane & 15, g = lane >> 4;
  const __bf16* const f = a.s + (size_t)b * N * a.ld_s + comp * a.Ds;
  const bf16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
  const unsigned foff = (unsigned)(tid >> 3) * (unsigned)a.ld_s + (tid & 7) * 8;
  bf16x8 pf[4];
  auto gload = [&](int c) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int row = (tid >> 3) + u * 64;        // (uniform chunk / trip base + one lane offset: row 64 u + tid / 8, piece tid % 8)
      pf[u] = (row < RF_SLD && row < N) ? *(const bf16x8*)((f + c * 64 + (size_t)u * 64 * a.ld_s) + foff) : zero;
    }
  };
  auto lstore = [&](int stage) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int sg = tid + u * 512, row = sg >> 3, piece = sg & 7;
      if (sg < RB_SEGS) *(bf16x8*)(lds + stage * RB_STAGE + row * RF_STRIDE + piece * 16) = pf[u];
    }
  };
  gload(0);
  // every element of S was written by the forward: all 208 rows x 224 columns are read
  const __bf16* const Sl = a.S + (((size_t)comp * a.B + b) * RF_ROWS + wave * 16 + n) * RF_SLD + g * 8;
  bf16x8 sf[2][7];
#pragma unroll
  for (int ks = 0; ks < 7; ++ks) {
    sf[0][ks] = *(const bf16x8*)(Sl + ks * 32);
    sf[1][ks] = two ? *(const bf16x8*)(Sl + (size_t)128 * RF_SLD + ks * 32) : zero;
  }
  lstore(0);
  __syncthreads();
  const float up = a.upstream[comp];
  // transposed read: lane 4 q + p of a 16-lane group addresses row q, columns 4 p .. 4 p + 3 of a 4 x 16 block and receives column (lane & 15)
  const int trd = (8 * g + (n >> 2)) * RF_STRIDE + (n & 3) * 8;
  for (int c = 0; c < nch; ++c) {
    if (c + 1 < nch) gload(c + 1);
    const char* const st = lds + (c & 1) * RB_STAGE + trd;
    f32x4 acc[2][4];
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) acc[h][ct] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < 7; ++ks) {
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) {
        const char* p = st + ks * 32 * RF_STRIDE + ct * 32;
        const bf16x8 ff = cat8(lds_tr_read(p), lds_tr_read(p + 4 * RF_STRIDE));
        acc[0][ct] = mfma16(ff, sf[0][ks], acc[0][ct]);
        if (two) acc[1][ct] = mfma16(ff, sf[1][ks], acc[1][ct]);
      }
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int i = (wave + 8 * h) * 16 + n;
      if ((h == 0 || two) && i < N) {
        __bf16* const o = a.d + ((size_t)b * N + i) * a.ld_d + comp * a.Ds + c * 64 + 4 * g;
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) {
          const f32x4 v = acc[h][ct];
          *(bf16x4*)(o + ct * 16) = (bf16x4){f2bf(v[0] * up), f2bf(v[1] * up), f2bf(v[2] * up), f2bf(v[3] * up)};
        }
      }
    }
    if (c + 1 < nch) lstore((c + 1) & 1);
    __syncthreads();
  }
}

bool rel_fused_shape_ok(int B, int N, int D, int ld) {
  return B > 0 && N > 0 && N <= RF_ROWS && D > 0 && D <= 1024 && D % 64 == 0 && ld >= 3 * D && ld % 8 == 0;
}

}  // namespace

extern "C" int devit_relation_fused_fwd(const void* s_qkv, const void* t_qkv, int B, int N, int Ds, int Dt, int ld_s, int ld_t,
                                        int head_dim_t, int head_dim_s, int teacher_f16, float* lse_t, float* lse_s, float* row_kl,
                                        void* S_out, float* loss3, void* stream) {
  DEVIT_CHECK(s_qkv && t_qkv && lse_t && lse_s && row_kl && S_out && loss3, DEVIT_ERR_ARG, "devit_relation_fused_fwd: null pointer");
  DEVIT_CHECK(((uintptr_t)s_qkv | (uintptr_t)t_qkv | (uintptr_t)S_out) % 16 == 0, DEVIT_ERR_ARG,
              "devit_relation_fused_fwd: the qkv buffers and S must be 16-byte aligned");
  DEVIT_CHECK(rel_fused_shape_ok(B, N, Ds, ld_s) && rel_fused_shape_ok(B, N, Dt, ld_t) && head_dim_t > 0 && head_dim_s > 0 &&
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
  hipLaunchKernelGGL(rel_fused_reduce_kernel, dim3(3), dim3(1024), 0, (hipStream_t)stream, (const float*)row_kl, B * N, 1.0f / (float)B, loss3);
  DEVIT_LAUNCH_CHECK();
  return DEVIT_OK;
}

extern "C" int devit_relation_fused_bwd(const void* S, const void* s_qkv, const float* upstream3, int B, int N, int Ds, int ld_s, void* d,
                                        int ld_d, void* stream) {
  DEVIT_CHECK(S && s_qkv && upstream3 && d, DEVIT_ERR_ARG, "devit_relation_fused_bwd: null pointer");
  DEVIT_CHECK(((uintptr_t)S | (uintptr_t)s_qkv) % 16 == 0 && (uintptr_t)d % 8 == 0, DEVIT_ERR_ARG,
              "devit_relation_fused_bwd: S and the qkv buffer must be 16-byte aligned, d 8-byte aligned");
  DEVIT_CHECK(rel_fused_shape_ok(B, N, Ds, ld_s) && ld_d >= 3 * Ds && ld_d % 4 == 0, DEVIT_ERR_SHAPE,
              "devit_relation_fused_bwd: B=%d N=%d Ds=%d ld_s=%d ld_d=%d: N <= 208, Ds a multiple of 64 up to 1024, ld_s a multiple of 8, ld_d of 4, "
              "both >= 3 Ds",
              B, N, Ds, ld_s, ld_d);
  RelFusedBwdArgs a{(const __bf16*)S, (const __bf16*)s_qkv, upstream3, (__bf16*)d, B, N, Ds, ld_s, ld_d};
  hipLaunchKernelGGL(rel_fused_bwd_kernel, dim3(B, 3), dim3(512), 0, (hipStream_t)stream, a);
  DEVIT_LAUNCH_CHECK();
  return DEVIT_OK;
}
