// The per-row arithmetic of the LayerNorm backward, in ONE place: layernorm.hip's standalone kernel and the full-row GEMM's fused epilogue
// (gemmfr.hip) both run these bodies in the same lane layout -- half a wave (32 lanes) per token row, lane l holds float4 v of the row at columns
// (v * 32 + l) * 4 -- with the same order of additions and the same xor-shuffle tree, so a row comes out bit for bit the same whichever
// kernel handled it (tests/test_gpu_lnfuse.py; tests/test_gpu_fullsize.py switches the full-row kernel, and with it the fusion, on and off).
#pragma once
#include "devit_common.h"

struct LnBwdArgs {
  const void* dy;       // [rows][D] bf16 or f32 (dense, row r); the fused epilogue takes dy from the GEMM's own tile instead
  const float* x;       // forward input, physical row map as in fwd
  const float* mean;
  const float* rstd;
  const float* gamma;
  const float* dres;    // [phys rows][D] f32 upstream residual-stream gradient or NULL
  float* dx;            // [phys rows][D] f32 = dres + LN'(dy)
  __bf16* dx_bf16;      // optional bf16 copy of rowscale * dx (branch gradient for the next GEMMs)
  const float* rowscale;
  int rows_per_scale;
  float* partial;       // [parts][3][D] column partial sums (dgamma, dbeta, colsum of dx_bf16)
  int rows, D, in_group, in_stride, dy_is_f32;
};

__device__ __forceinline__ size_t ln_in_row(int r, int group, int stride) {
  return group > 0 ? (size_t)(r / group) * stride + (r % group) : (size_t)r;
}

// what a half-wave carries across its rows: gamma and the three column sums of its 4 * NV columns
template <int NV>
struct LnBwdCols {
  f32x4 gm[NV], dg[NV], db[NV], dsum[NV];
  bool ok[NV];
};

// one row's inputs as the half-wave holds them (zeros where the row, or the lane's float4 of it, does not exist)
template <int NV>
struct LnBwdRow {
  f32x4 xv[NV], dyv[NV];
  float mu, rs;
};

// (zero: the fused epilogue passes a zero the compiler cannot see through, so that thirty-six constants are not kept in registers across its K loop)
template <int NV, bool RAG>
__device__ __forceinline__ void ln_bwd_cols_init(const LnBwdArgs& a, int hl, LnBwdCols<NV>& s, f32x4 zero = (f32x4){0.f, 0.f, 0.f, 0.f}) {
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    s.ok[v] = !RAG || v * 128 + hl * 4 < a.D;
    s.gm[v] = s.ok[v] ? *(const f32x4*)(a.gamma + v * 128 + hl * 4) : zero;
    s.dg[v] = zero;
    s.db[v] = zero;
    s.dsum[v] = zero;
  }
}

// __shfl_xor over the wave with the caller's lane index (the same ds_bpermute; the fused epilogue must not keep a lane index of its own alive
// across its K loop)
__device__ __forceinline__ float ln_shfl_xor(float v, int o, int lane) {
  return __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute((lane ^ o) << 2, __builtin_bit_cast(int, v)));
}

// The floating-point expressions of a row.  The general form leaves the choice of fused multiply-adds to hipcc (-ffp-contract=fast-honor-pragmas):
// what it chose is part of the kernel's results.
template <int NV, bool RAG>
struct LnBwdMath {
  // xh = (x - mean) * rstd, g = dy * gamma, the lane's share of s1 = sum g and s2 = sum g * xh, and the column sums dgamma += dy * xh, dbeta += dy
  static __device__ __forceinline__ void sums(const LnBwdRow<NV>& in, LnBwdCols<NV>& s, f32x4 (&xh)[NV], f32x4 (&g)[NV], float& s1, float& s2) {
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      xh[v] = s.ok[v] ? (in.xv[v] - in.mu) * in.rs : (f32x4){0.f, 0.f, 0.f, 0.f};
      g[v] = in.dyv[v] * s.gm[v];
      s.dg[v] += in.dyv[v] * xh[v];
      s.db[v] += in.dyv[v];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        s1 += g[v][e];
        s2 += g[v][e] * xh[v][e];
      }
    }
  }
  // rstd * (g - mean(g) - xh * mean(g * xh)) of the lane's float4 v; s1, s2 are the row's sums
  static __device__ __forceinline__ f32x4 dx(int v, const f32x4& g, const f32x4& xh, float s1, float s2, float invD, float rs) {
    const float m1 = s1 * invD, m2 = s2 * invD;
    return rs * (g - m1 - xh * m2);
  }
};
// D = 384 (the student: the rows the fused epilogue also handles) with every operation pinned, so that the two kernels cannot drift apart through a
// contraction hipcc makes in one context and not in the other.  The operations are the ones the standalone kernel's code object held when the fused
// epilogue was written (s2 and dgamma accumulate by fused multiply-add; the first float4 takes g - s1 / D as one fused operation, the others subtract
// the rounded mean; xh * m2 is subtracted by fused multiply-add): its results are unchanged.
template <>
struct LnBwdMath<3, false> {
  static __device__ __forceinline__ void sums(const LnBwdRow<3>& in, LnBwdCols<3>& s, f32x4 (&xh)[3], f32x4 (&g)[3], float& s1, float& s2) {
#pragma clang fp contract(off)
#pragma unroll
    for (int v = 0; v < 3; ++v) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        xh[v][e] = (in.xv[v][e] - in.mu) * in.rs;
        g[v][e] = in.dyv[v][e] * s.gm[v][e];
        s.dg[v][e] = __builtin_fmaf(in.dyv[v][e], xh[v][e], s.dg[v][e]);
        s.db[v][e] += in.dyv[v][e];
        s1 += g[v][e];
        s2 = __builtin_fmaf(g[v][e], xh[v][e], s2);
      }
    }
  }
  static __device__ __forceinline__ f32x4 dx(int v, const f32x4& g, const f32x4& xh, float s1, float s2, float invD, float rs) {
#pragma clang fp contract(off)
    const float m1 = s1 * invD, m2 = s2 * invD;
    f32x4 d;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float t = v == 0 ? __builtin_fmaf(-invD, s1, g[e]) : g[e] - m1;
      d[e] = rs * __builtin_fmaf(-m2, xh[e], t);
    }
    return d;
  }
};

// One row of the LayerNorm backward.  Every lane of the wave must call it (the shuffles; lane = its index in the wave, hl = lane & 31); `live` =
// the half-wave's row exists, pr = its physical row, D = a.D (a constant where the caller has one), rsc = the row's scale of dx_bf16 (1 without).
// dres_at(v, o) returns the float4 of dres at element offset o (called only when a.dres is set): a load in the standalone kernel, a
// register the epilogue fetched ahead in the fused one.
template <int NV, bool RAG, typename DRES>
__device__ __forceinline__ void ln_bwd_row(const LnBwdArgs& a, LnBwdCols<NV>& s, const LnBwdRow<NV>& in, bool live, size_t pr, int lane,
                                           int D, float invD, float rsc, DRES&& dres_at) {
  const int hl = lane & 31;
  f32x4 xh[NV], g[NV];
  float s1 = 0.f, s2 = 0.f;
  LnBwdMath<NV, RAG>::sums(in, s, xh, g, s1, s2);
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) {
    s1 += ln_shfl_xor(s1, o, lane);
    s2 += ln_shfl_xor(s2, o, lane);
  }
  if (live) {
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      const size_t o = pr * D + v * 128 + hl * 4;
      if (RAG && !s.ok[v]) continue;
      f32x4 d = LnBwdMath<NV, RAG>::dx(v, g[v], xh[v], s1, s2, invD, in.rs);
      if (a.dres) {
        // (the residual is added to the ROUNDED product wherever it comes from: a register operand must not turn this into a fused multiply-add
        // that the standalone kernel, whose add sits behind a load, does not have)
        asm volatile("" : "+v"(d));
        d += dres_at(v, o);
      }
      *(f32x4*)(a.dx + o) = d;
      if (a.dx_bf16) {
        const bf16x4 ob = {f2bf(d[0] * rsc), f2bf(d[1] * rsc), f2bf(d[2] * rsc), f2bf(d[3] * rsc)};
        *(bf16x4*)(a.dx_bf16 + o) = ob;
        s.dsum[v] += (f32x4){bf2f(ob[0]), bf2f(ob[1]), bf2f(ob[2]), bf2f(ob[3])};
      }
    }
  }
}

// Column sums of a 256-thread workgroup -> partial[part][{dgamma, dbeta, colsum(dx_bf16)}][D], in a fixed order: the two half-waves of a wave,
// then the four waves.  red: [4][3][NV * 128] floats of LDS.
template <int NV>
__device__ __forceinline__ void ln_bwd_cols_store(const LnBwdArgs& a, LnBwdCols<NV>& s, float (*red)[3][NV * 128], int wv, int lane,
                                                  int D, size_t part) {
  const int hl = lane & 31, half = lane >> 5, tid = wv * 64 + lane;
#pragma unroll
  for (int v = 0; v < NV; ++v) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {      // the two half-waves hold the same columns
      s.dg[v][e] += ln_shfl_xor(s.dg[v][e], 32, lane);
      s.db[v][e] += ln_shfl_xor(s.db[v][e], 32, lane);
      s.dsum[v][e] += ln_shfl_xor(s.dsum[v][e], 32, lane);
    }
    if (half == 0 && s.ok[v]) {
      *(f32x4*)&red[wv][0][v * 128 + hl * 4] = s.dg[v];
      *(f32x4*)&red[wv][1][v * 128 + hl * 4] = s.db[v];
      *(f32x4*)&red[wv][2][v * 128 + hl * 4] = s.dsum[v];
    }
  }
  __syncthreads();
  for (int i = tid; i < 3 * D; i += 256) {
    const int which = i / D, c = i - which * D;
    a.partial[(part * 3 + which) * D + c] = red[0][which][c] + red[1][which][c] + red[2][which][c] + red[3][which][c];
  }
}
