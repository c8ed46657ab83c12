// bf16 MFMA GEMM for gfx950 with fused epilogues.  C[M,N] = sum_k A(m,k) B(n,k).
//
// Tiles 128x128x64 (4 waves, two workgroups per CU) or 256x256x64 (8 waves), each wave a 64x64 / 128x64 sub-tile of
// MFMA 16x16x32 accumulators.  Operand tiles go HBM -> LDS by LDS-DMA (global_load_lds_dwordx4, 1 KiB per
// wave-instruction) into a two-stage ring: the next stage is in flight while the current one is multiplied.  The
// LDS image is lane-linear, so the bank-conflict swizzle is applied to the per-lane SOURCE
// address and undone by the same XOR on the fragment read (cdna_hip_programming.md §5.4 rule 21): swz_row() for
// k-contiguous operands (ds_read_b128 fragments), swz_krow() for k-major operands (ds_read_b64_tr_b16 fragments).
// Epilogues run straight from the accumulators (epilogue_direct): the MFMAs take the weight operand on their row
// side so each lane owns consecutive output columns; only the split-K atomic epilogue stages through LDS.
// This header: the device code the kernels share -- LDS-DMA staging, images, swizzles, fragment reads, the register epilogues, the tile order.
// Three kernels share the images, swizzles, epilogue code and accumulation order (bit-identical results wherever two of them can run a launch):
// gemm_kernel (gemm_tile.h: eight waves, 128x128 / 256x256 ping-pong), gemm4_kernel (gemm4.hip: four waves, 256x256, generated asm K loop) and
// gemmfr_kernel (gemmfr.hip: four waves, full-row 256x384 for N = 384 outputs with a k-major weight, generated asm K loop); wgradfr_kernel
// (wgradfr.hip) runs the full-row tile on two k-major operands.  Host side (argument checks, kernel selection, C ABI): gemm.hip.
#pragma once
#include <type_traits>

#include "gemm_host.h"

namespace {

using devit_gemm::BK;
using devit_gemm::FastDiv;

__device__ __forceinline__ int fdiv(int n, const FastDiv& f) {
  return (int)(((unsigned long long)(unsigned)n * f.mul) >> f.shift);
}

// The kernels' argument: devit_gemm::GemmParams under a name of this (anonymous) namespace, where the kernels live -- their mangled names carry it
struct GemmArgs : devit_gemm::GemmParams {};

__device__ __forceinline__ int phys_row(int r, int group, int skip) {
  return group > 0 ? r + skip * (r / group + 1) : r;
}

// LDS image swizzles (applied to the DMA's source address and again on the fragment reads; the LDS side of an LDS-DMA
// is lane-linear).  16-byte chunk index XOR:
//   row-major image [rows][64 k], 128-B rows: by row bits (1, 2^4, 3) -- conflict-free ds_read_b128 both for 16
//     consecutive rows and for the PAIRED row set {0-3, 8-11, 16-19, 24-27} (+4 for odd tiles), see tile_row();
//   k-major image [64 k][W], read by ds_read_b64_tr_b16 (lane 4q+p: k-row q, four columns): k-row bits (0,1) go to
//     chunk bits (2,3) and k-row bit 3 to chunk bit 1 -- the sixteen 8-byte pieces of a 16-lane group land on distinct
//     banks whether its four column groups are adjacent (natural) or 16 bytes apart (PAIRED); k-rows r and r+4 share it.
__device__ __forceinline__ int swz_row(int row) { return ((row >> 1) & 7) ^ (((row >> 4) & 1) << 1); }
__device__ __forceinline__ int swz_krow(int krow) { return ((krow & 3) << 2) | (((krow >> 3) & 1) << 1); }

// Issue this wave's LDS-DMA loads (1 KiB each) for one operand tile of width W (128 or 256).
//   KM == false: operand stored [R][K]; `org` = &op[row0][0]; LDS image [W rows][64 k] (128-B rows)
//   KM == true : operand stored [K][R]; `org` = &op[0][col0]; LDS image [64 k][W cols] (2W-B rows)
// The address is split into a wave-uniform base that advances with k0 (SGPRs) and a per-lane 32-bit byte offset
// that is loop-invariant, so the K-loop issues `global_load_lds_dwordx4 voff, s[base]` with no per-step VALU math.
template <bool KM, int W, int NWAVES>
__device__ __forceinline__ unsigned lane_offset(int ld, int wave, int lane, int i, int valid) {
  // `valid` (<= W, a multiple of 8): operand rows (columns if k-major) of this tile that exist; the LDS image rows past
  // them are filled from the last existing one (a ragged last n-tile: their products are never stored)
  constexpr int CNT = (W / 8) / NWAVES;
  const int slab = wave * CNT + i;
  if (!KM) {
    const int row = slab * 8 + (lane >> 3);
    const int chunk = (lane & 7) ^ swz_row(row);
    return (unsigned)(min(row, valid - 1) * ld + chunk * 8) * 2u;
  } else {
    constexpr int LPR = W / 8, RPS = 64 / LPR;  // lanes per k-row, k-rows per 1-KiB slab
    const int krow = slab * RPS + lane / LPR;
    const int chunk = (lane % LPR) ^ swz_krow(krow);
    return (unsigned)(krow * ld + min(chunk, valid / 8 - 1) * 8) * 2u;
  }
}

// Two LDS-DMA instructions (16 B per lane, 1 KiB per wave-instruction) into consecutive 1-KiB slabs at LDS byte
// address `lds`.  Inline asm on purpose: hipcc's waitcnt pass treats a builtin LDS-DMA as a pending LDS write and
// guards later ds_reads with `s_waitcnt vmcnt(0)` whenever it cannot prove the buffers distinct -- which serialises
// the ring (observed: every K-step of some instantiations, every tile boundary of all).  Hidden in asm, the DMA is
// ordered by this kernel's own vmcnt wait + barrier (advance()); hipcc's counts for its own loads/stores stay
// safe because they can only be stricter with extra operations in the queue.  M0 (the DMA's LDS base) is saved and
// restored around the statement; the padding covers SGPR-write -> VMEM-read and M0-write -> LDS-DMA wait states
// (cdna_hip_programming.md §5.7).
template <bool NT = false>
__device__ __forceinline__ void dma2_uniform(const char* ubase, unsigned off0, unsigned off1, unsigned lds) {
  unsigned keep;
  if (NT) {
    asm volatile(
        "s_mov_b32 %0, m0\n\t"
        "s_mov_b32 m0, %1\n\t"
        "s_nop 2\n\t"
        "global_load_lds_dwordx4 %3, %2 nt\n\t"
        "s_add_u32 m0, %1, 0x400\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %4, %2 nt\n\t"
        "s_mov_b32 m0, %0"
        : "=&s"(keep)
        : "s"(lds), "s"(ubase), "v"(off0), "v"(off1)
        : "memory", "scc");
    return;
  }
  asm volatile(
      "s_mov_b32 %0, m0\n\t"
      "s_mov_b32 m0, %1\n\t"
      "s_nop 2\n\t"
      "global_load_lds_dwordx4 %3, %2\n\t"
      "s_add_u32 m0, %1, 0x400\n\t"
      "s_nop 0\n\t"
      "global_load_lds_dwordx4 %4, %2\n\t"
      "s_mov_b32 m0, %0"
      : "=&s"(keep)
      : "s"(lds), "s"(ubase), "v"(off0), "v"(off1)
      : "memory", "scc");
}
__device__ __forceinline__ void dma2_perlane(const void* p0, const void* p1, unsigned lds) {
  unsigned keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\t"
      "s_mov_b32 m0, %1\n\t"
      "s_nop 2\n\t"
      "global_load_lds_dwordx4 %2, off\n\t"
      "s_add_u32 m0, %1, 0x400\n\t"
      "s_nop 0\n\t"
      "global_load_lds_dwordx4 %3, off\n\t"
      "s_mov_b32 m0, %0"
      : "=&s"(keep)
      : "s"(lds), "v"(p0), "v"(p1)
      : "memory", "scc");
}

template <bool KM, int W, int NWAVES, bool NT = false>
__device__ __forceinline__ void stage_tile(const __bf16* org, int ld, int k0, int group, int skip,
                                           char* lds_tile, int wave, int lane, int valid = W) {
  constexpr int CNT = (W / 8) / NWAVES;
  static_assert(CNT % 2 == 0, "slabs are issued in pairs");
  const unsigned lds0 = (unsigned)(size_t)LDS_PTR(lds_tile) + (unsigned)(wave * CNT) * 1024u;
  if (KM && group > 0) {   // row-remapped reduction index (patch-embed wgrad): per-lane physical rows, generic path
#pragma unroll
    for (int i = 0; i < CNT; i += 2) {
      const __bf16* src[2];
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        constexpr int LPR = W / 8, RPS = 64 / LPR;
        const int slab = wave * CNT + i + e;
        const int krow = slab * RPS + lane / LPR;
        const int chunk = (lane % LPR) ^ swz_krow(krow);
        src[e] = org + (size_t)phys_row(k0 + krow, group, skip) * ld + chunk * 8;
      }
      dma2_perlane(src[0], src[1], lds0 + i * 1024u);
    }
    return;
  }
  const char* ubase = (const char*)org + (size_t)k0 * (KM ? (size_t)ld : (size_t)1) * 2;   // wave-uniform
#pragma unroll
  for (int i = 0; i < CNT; i += 2)
    dma2_uniform<NT>(ubase, lane_offset<KM, W, NWAVES>(ld, wave, lane, i, valid), lane_offset<KM, W, NWAVES>(ld, wave, lane, i + 1, valid),
                     lds0 + i * 1024u);
}

// Offset, inside a 64-wide wave tile, of operand row p (0..15) of 16-row tile j.  PAIRED interleaves tiles 2q and
// 2q+1 in groups of four so that, with the operand on the MFMA's row side, lane group g = lane>>4 (which receives
// rows 4g..4g+3 of every tile) ends up with EIGHT consecutive columns of the output per tile pair: one 16-byte bf16
// store.  The natural order gives four consecutive columns per tile: one 16-byte fp32 store.
template <bool PAIRED>
__device__ __forceinline__ int tile_row(int j, int p) {
  return PAIRED ? 32 * (j >> 1) + 8 * (p >> 2) + 4 * (j & 1) + (p & 3) : 16 * j + p;
}

// One MFMA operand fragment: 16-row tile j of the wave's operand rows starting at `base` of the W-wide LDS tile,
// k-step kk of 2.
template <bool KM, int W, bool PAIRED>
__device__ __forceinline__ bf16x8 read_frag(const char* tile, int base, int j, int kk, int lane) {
  if (!KM) {
    const int row = base + tile_row<PAIRED>(j, lane & 15);
    const int chunk = (kk * 4 + (lane >> 4)) ^ swz_row(row);
    return *(const bf16x8*)(tile + row * 128 + chunk * 16);
  } else {
    const int G = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
    const int col0 = base + tile_row<PAIRED>(j, 4 * p);   // this lane addresses operand rows 4p..4p+3 of k-row q
    const int krow = kk * 32 + G * 8 + q;
    const int chunk = (col0 >> 3) ^ swz_krow(krow);
    const char* a = tile + krow * (W * 2) + chunk * 16 + ((col0 >> 2) & 1) * 8;
    return cat8(lds_tr_read(a), lds_tr_read(a + 4 * (W * 2)));
  }
}

template <int N>
__device__ __forceinline__ void wait_vmcnt() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// Fused epilogue straight from the accumulators.  The K loop runs the MFMAs with the weight operand on the row side,
// so lane (g = lane>>4, c = lane&15) holds, for m-tile i and n-tile j, C[m = 16 i + c][n = tile_row(j, 4g + r)],
// r = 0..3: consecutive output columns in consecutive registers.  Every global access is 16 bytes per lane (8 for the
// optional bf16 copy of the RESIDUAL kind) and the four lane groups of a row cover 64 contiguous bytes.  Rows are
// handled two m-tiles at a time in two phases -- the chunk's global inputs (residual / saved pre-activation /
// pos-embed) first, then compute + stores -- so that no load queues behind the stores of an earlier row (vmcnt counts
// loads and stores in order on gfx950).  No LDS is touched: the operand ring is free while the epilogue runs.
// FULL = every row of the tile is a real row (m < m_lim): no predicates.
// Epilogue output store: plain.  Measured (tools/gemm_bench.py + bench.py A/B): write-through (sc1) stores -12 % on the
// GEMM itself; non-temporal stores +2..7 % on the bf16-output GEMMs and -1..11 % on the fp32 residual ones, and no
// change of the step time (the consumer kernels pay what the producers gain).
template <typename T>
__device__ __forceinline__ void st_out(T* p, T v) {
#ifdef DEVIT_GEMM_NOSTORE   // diagnostic build: the epilogue computes everything and stores (almost) nothing
  if (__builtin_expect(((size_t)p & 0xfffff0) == 0x7ffff0, 0))
#endif
  *p = v;
}

template <bool F16 = false>
__device__ __forceinline__ bf16x8 pack8(const float (&x)[8]) {
  if constexpr (F16) return cvt8<true>((f32x4){x[0], x[1], x[2], x[3]}, (f32x4){x[4], x[5], x[6], x[7]});
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
  bf16x2 p[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) p[e] = __builtin_convertvector((f32x2){x[2 * e], x[2 * e + 1]}, bf16x2);   // v_cvt_pk_bf16_f32
  return (bf16x8){p[0][0], p[0][1], p[1][0], p[1][1], p[2][0], p[2][1], p[3][0], p[3][1]};
}

// Per-lane column data of an epilogue: the lane's four column offsets (one per n-tile) and bias / column scale there.
template <int KIND>
__device__ __forceinline__ void load_cols(const devit_epilogue& ep, int lane, int nw, int (&noff)[4], f32x4 (&bias)[4],
                                          f32x4 (&cs)[4]) {
  constexpr bool BF16_OUT = KIND == DEVIT_EPI_STORE_BF16 || KIND == DEVIT_EPI_GELU_BF16 || KIND == DEVIT_EPI_DGELU_BF16;
  constexpr bool SCALED = KIND == DEVIT_EPI_GELU_BF16 || KIND == DEVIT_EPI_DGELU_BF16;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    noff[j] = nw + tile_row<BF16_OUT>(j, 4 * (lane >> 4));
    // (the dGELU kind is a dgrad: no bias by contract, checked on the host -- 16 registers the 255-VGPR 256x256 instantiation
    // does not have: it spilled 4 to scratch with them, and scratch reloads inside a K-step land in the counted vmcnt waits)
    if constexpr (KIND == DEVIT_EPI_DGELU_BF16) bias[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    else bias[j] = ep.bias ? *(const f32x4*)(ep.bias + noff[j]) : (f32x4){0.f, 0.f, 0.f, 0.f};
    if (SCALED) cs[j] = ep.colscale ? *(const f32x4*)(ep.colscale + noff[j]) : (f32x4){1.f, 1.f, 1.f, 1.f};
  }
}
// Make hipcc wait for the loads of load_cols() HERE (an empty asm that reads them).  Its waitcnt pass does not see
// the asm LDS-DMA: a wait it places after the next DMA issue would also wait for that DMA.
template <int KIND>
__device__ __forceinline__ void settle_cols(f32x4 (&bias)[4], f32x4 (&cs)[4]) {
  constexpr bool SCALED = KIND == DEVIT_EPI_GELU_BF16 || KIND == DEVIT_EPI_DGELU_BF16;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (KIND != DEVIT_EPI_DGELU_BF16) asm volatile("" : "+v"(bias[j]));
    if (SCALED) asm volatile("" : "+v"(cs[j]));
  }
}

// The fp32-output kinds (STORE_F32, PATCH_F32, RESIDUAL_F32) with whole 128-byte rows per memory instruction.  Lane (g, c)
// holds, per n-tile j, four consecutive floats of row c at column 16 j + 4 g: one instruction per n-tile touches 16 rows x
// 64 bytes -- half cache lines, twice the transactions of the bytes moved, on an epilogue that runs at the CU's transaction
// rate.  Here the n-tiles (2 p, 2 p + 1) of a row are one 128-byte line: lanes c and c ^ 8 trade a chunk (swap_half_rows)
// so that instruction A covers rows 0-7 and instruction B rows 8-15 of the m-tile, every row a whole line; the residual /
// pos-embed inputs are fetched in that same shape.  Same arithmetic per element as the earlier 64-byte-half form (one instruction per
// n-tile; profiles/r03_A_f32_full_rows.txt measured the two; that form is in the git history).
template <int KIND, int MI, bool FULL, bool F16>
__device__ __forceinline__ void epilogue_f32_rows(const devit_epilogue& ep, f32x4 (&acc)[MI][4], const int (&noff)[4],
                                                  const f32x4 (&bias)[4], int lane, int mw, int m_lim, size_t ob) {
  constexpr int CHI = 2;
  const int c = lane & 15;
  const bool hi = c >= 8;
  const int colx = hi ? 16 : 0;                     // floats: second half of the line
  auto row_off = [&](int m, int& tok) -> size_t {   // element offset of output row m (PATCH: token remap)
    if (KIND == DEVIT_EPI_PATCH_F32) {
      const int b = m / ep.patch_tokens, t = m - b * ep.patch_tokens;
      tok = ep.extra_tokens + t;
      return ((size_t)b * (ep.patch_tokens + ep.extra_tokens) + tok) * ep.ldc;
    }
    tok = 0;
    return ob + (size_t)m * ep.ldc;
  };
#pragma unroll
  for (int i0 = 0; i0 < MI; i0 += CHI) {
    // ---- phase 1: global inputs of the chunk, in the shape they will be stored in
    f32x4 gin[CHI][2][2];          // [m-tile][line p][rows 0-7 / 8-15]
    float rsc[CHI][2];
    size_t rowo[CHI][2];
    bool okr[CHI][2];
#pragma unroll
    for (int u = 0; u < CHI; ++u)
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        const int m = mw + (i0 + u) * 16 + (c & 7) + 8 * r;
        const bool ok = FULL || m < m_lim;
        int tok;
        const size_t o = row_off(m, tok);
#pragma unroll
        for (int p = 0; p < 2; ++p) {
          const int col = noff[2 * p] + colx;
          if (KIND == DEVIT_EPI_PATCH_F32)
            gin[u][p][r] = ok ? *(const f32x4*)(ep.pos + (size_t)tok * ep.ldc + col) : (f32x4){0.f, 0.f, 0.f, 0.f};
          if (KIND == DEVIT_EPI_RESIDUAL_F32)
            gin[u][p][r] = ok ? load_stream((const f32x4*)(ep.res + o + col)) : (f32x4){0.f, 0.f, 0.f, 0.f};
        }
        if (KIND == DEVIT_EPI_RESIDUAL_F32) rsc[u][r] = (ok && ep.rowscale) ? ep.rowscale[m / ep.rows_per_scale] : 1.0f;
        rowo[u][r] = o;
        okr[u][r] = ok;
      }
    // ---- phase 2: compute + store
#pragma unroll
    for (int u = 0; u < CHI; ++u) {
      const int i = i0 + u;
      f32x4 v[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = acc[i][j] + bias[j];
      if (KIND == DEVIT_EPI_RESIDUAL_F32 && ep.aux) {   // optional bf16 copy of the branch output (output_att): row c, 8 bytes per lane
        const int m = mw + i * 16 + c;
        if (FULL || m < m_lim) {
#pragma unroll
          for (int j = 0; j < 4; ++j) st_out((bf16x4*)((__bf16*)ep.aux + ob + (size_t)m * ep.ldc + noff[j]), cvt4<F16>(v[j]));
        }
      }
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        swap_half_rows(v[2 * p], v[2 * p + 1], hi);
        const int col = noff[2 * p] + colx;
#pragma unroll
        for (int r = 0; r < 2; ++r) {
          f32x4 w = v[2 * p + r];
          if (KIND == DEVIT_EPI_PATCH_F32) w = w + gin[u][p][r];
          if (KIND == DEVIT_EPI_RESIDUAL_F32) w = gin[u][p][r] + rsc[u][r] * w;
          if (okr[u][r]) st_out((f32x4*)((float*)ep.out + rowo[u][r] + col), w);
        }
      }
    }
  }
}

template <int KIND, int MI, bool FULL, bool F16 = false>
__device__ __forceinline__ void epilogue_direct(const devit_epilogue& ep, f32x4 (&acc)[MI][4], const int (&noff)[4],
                                                const f32x4 (&bias)[4], const f32x4 (&cs)[4], int lane, int mw,
                                                int m_lim, size_t ob) {
  constexpr bool BF16_OUT = KIND == DEVIT_EPI_STORE_BF16 || KIND == DEVIT_EPI_GELU_BF16 || KIND == DEVIT_EPI_DGELU_BF16;
  if constexpr (!BF16_OUT) {
    epilogue_f32_rows<KIND, MI, FULL, F16>(ep, acc, noff, bias, lane, mw, m_lim, ob);
    return;
  }
  constexpr int CHI = 2;
  const int c = lane & 15;
#pragma unroll
  for (int i0 = 0; i0 < MI; i0 += CHI) {
    // ---- phase 1: global inputs of the chunk
    bf16x8 pre[CHI][2];
#pragma unroll
    for (int u = 0; u < CHI; ++u) {
      const int m = mw + (i0 + u) * 16 + c;
      const bool ok = FULL || m < m_lim;
      const size_t o = ob + (size_t)m * ep.ldc;
      if (KIND == DEVIT_EPI_DGELU_BF16) {
        const bf16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int q = 0; q < 2; ++q)
          pre[u][q] = ok ? load_stream((const bf16x8*)((const __bf16*)ep.aux_in + o + noff[2 * q])) : z;
      }
    }
    // ---- phase 2: compute + store
#pragma unroll
    for (int u = 0; u < CHI; ++u) {
      const int i = i0 + u;
      bf16x8 outc[2], prec[2];
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        float x[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) x[e] = acc[i][2 * q + (e >> 2)][e & 3] + bias[2 * q + (e >> 2)][e & 3];
        if (KIND == DEVIT_EPI_GELU_BF16) {
          prec[q] = pack8<F16>(x);
#pragma unroll
          for (int e = 0; e < 8; ++e) x[e] = gelu_fwd<false>(x[e]) * cs[2 * q + (e >> 2)][e & 3];
        } else if (KIND == DEVIT_EPI_DGELU_BF16) {
#pragma unroll
          for (int e = 0; e < 8; ++e) x[e] = x[e] * cs[2 * q + (e >> 2)][e & 3] * gelu_bwd<false>(bf2f(pre[u][q][e]));
        }
        outc[q] = pack8<F16>(x);
      }
      // whole 128-byte rows per store: rows (c & 7) and 8 + (c & 7) of this m-tile, see swap_half_rows()
      const bool hi = c >= 8;
      const int mA = mw + i * 16 + (c & 7);
      const size_t oA = ob + (size_t)mA * ep.ldc + noff[0] + (hi ? 32 : 0), oB = oA + (size_t)8 * ep.ldc;
      const bool okA = FULL || mA < m_lim, okB = FULL || mA + 8 < m_lim;
      swap_half_rows(outc[0], outc[1], hi);
      if (KIND == DEVIT_EPI_GELU_BF16 && ep.aux) {
        swap_half_rows(prec[0], prec[1], hi);
        if (okA) st_out((bf16x8*)((__bf16*)ep.aux + oA), prec[0]);
        if (okB) st_out((bf16x8*)((__bf16*)ep.aux + oB), prec[1]);
      }
      if (okA) st_out((bf16x8*)((__bf16*)ep.out + oA), outc[0]);
      if (okB) st_out((bf16x8*)((__bf16*)ep.out + oB), outc[1]);
    }
  }
}

// Where one output tile's operands start and which K-steps it covers (all wave-uniform).
struct TileRef {
  const __bf16* a;
  const __bf16* b;
  int m0, n0, bz, kt0, nk;
};

template <int BM, int BN, bool A_KM, bool B_KM>
__device__ __forceinline__ TileRef decode_tile(const GemmArgs& g, int w) {
  const int zz = fdiv(w, g.d_per_z);
  const int r0 = w - zz * g.d_per_z.d;
  const int chunk = fdiv(r0, g.d_chunk);                // full chunks (gn n-tiles x all m-tiles) come first
  const int r1 = r0 - chunk * g.d_chunk.d;
  const bool lastc = (chunk + 1) * g.gn > g.tiles_n;    // the last chunk may be narrower
  const int tm = lastc ? fdiv(r1, g.d_last) : fdiv(r1, g.d_gn);
  const int tn = chunk * g.gn + r1 - tm * (lastc ? g.d_last.d : g.d_gn.d);
  const int bzq = fdiv(zz, g.d_split);
  const int z = zz - bzq * g.split_k, nk_total = g.K / BK;
  TileRef t;
  t.bz = bzq;
  t.m0 = tm * BM;
  t.n0 = tn * BN;
  t.kt0 = fdiv(z * nk_total, g.d_split);
  t.nk = fdiv((z + 1) * nk_total, g.d_split) - t.kt0;
  t.a = g.A + (size_t)t.bz * g.a_bs + (A_KM ? (size_t)t.m0 : (size_t)t.m0 * g.lda);
  t.b = g.B + (size_t)t.bz * g.b_bs + (B_KM ? (size_t)t.n0 : (size_t)t.n0 * g.ldb);
  return t;
}

// ---- the 384-wide k-major B stage of the full-row tile (gemmfr_kernel, wgradfr_kernel)
typedef float f32x32 __attribute__((ext_vector_type(32)));

// per-lane source byte offset of slab i (1 KiB, of this wave's twelve = 16 k rows) of a 384-wide k-major B stage, relative to the wave's
// first k row.  Image [64 k][384 cols]: a k-row is 48 chunks of 16 bytes, slabs cross k-rows (lane_offset<true> wants 64 % (W / 8) == 0).
__device__ __forceinline__ unsigned fr_dma_off_b(int ld, int wave, int lane, int i) {
  const int piece = (wave * 12 + i) * 64 + lane, krow = piece / 48, c = piece % 48;
  return (unsigned)((krow - 16 * wave) * ld + ((c ^ swz_krow(krow)) * 8)) * 2u;
}

// first k row of wave `wave`'s share (16 k rows) of B stage u: the stages are shifted by half a stage and cyclic in K
__device__ __forceinline__ int fr_b_row(int u, int wave, int K) {
  const int r = 64 * u - 32 + 16 * wave;
  return r < 0 ? r + K : (r >= K ? r - K : r);
}

}  // namespace
