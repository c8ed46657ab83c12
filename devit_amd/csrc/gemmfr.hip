// gemmfr_kernel, its fused LayerNorm-backward epilogue, and its launcher.
#include "gemm_device.h"
#include "ln_rows.h"

namespace {

// ---------------------------------------------------------------------------------------------------------------------
// Full-row 256x384x64 kernel (round 5): the student's N = 384 launches -- activation operand row-major, weight operand K-MAJOR (the
// dgrads of qkv / proj / fc1 as they stand; proj / fc2 forward through a k-major copy of their weights), bf16 store or fp32 residual
// epilogue.  Four waves, one per SIMD, each a 128 x 192 sub-tile = 96 accumulator tiles: 64 in a[0:255], 32 in v[128:255] (pinned asm
// outputs); ONE fragment buffer; two A slots (32 KB) + two B slots (48 KB), the B stages shifted by half a stage so that a slot is
// released -- and 8 or 12 requests per wave leave -- in EVERY phase; the K loop is a generated inline-asm statement
// (gemmfr_kloop.inc, tools/gen_gemmfr.py: register plan, ring protocol, operand list).  Same LDS images / swizzles / MFMA operand roles /
// accumulation order per output element as the 128x128 kernels these launches ran on: bit-identical results.  Why: two 128x128
// workgroups per CU ask the CU's fill path for 64 B per cycle of matrix pipe and get ~24; this tile needs
// 26.7 and reads the activation panel once instead of three times.
#include "gemmfr_kloop.inc"

// Internal epilogue kind of gemmfr_kernel (not a devit_epilogue kind): the bf16 store of DEVIT_EPI_STORE_BF16 goes to LDS instead of memory and the
// LayerNorm backward of those rows runs in the same workgroup (see the epilogue below).  One tile per workgroup only.
constexpr int DEVIT_EPI_LNBWD = 64;
template <int KIND>
struct FrArgs {
  GemmArgs g;
};
template <>
struct FrArgs<DEVIT_EPI_LNBWD> {
  GemmArgs g;
  LnBwdArgs ln;
};
constexpr int LNF_PITCH = 832;                  // bytes of a staged bf16 row: 768 + 64, so that the sixteen rows of an m-tile start in different banks
constexpr int LNF_ROWS = 128;                   // rows staged per pass (two passes per tile)
constexpr int LNF_RED = LNF_ROWS * LNF_PITCH;   // byte offset of the column sums' reduction buffer [4][3][384] floats
constexpr int LNF_SIDE = LNF_RED + 4 * 3 * 384 * 4, LNF_SIDE_PITCH = 272;   // the second pass's VGPR-resident columns: [128][2 x 64] bf16, rows 256 + 16 bytes
static_assert(LNF_SIDE + LNF_ROWS * LNF_SIDE_PITCH <= (256 + 384) * 128 * 2, "the fused epilogue lives in the operand ring's LDS");

template <int KIND>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1)))
void gemmfr_kernel(const FrArgs<KIND> fa) {
  static_assert(KIND == DEVIT_EPI_RESIDUAL_F32 || KIND == DEVIT_EPI_STORE_BF16 || KIND == DEVIT_EPI_LNBWD, "the student's N = 384 launches");
  const GemmArgs& g = fa.g;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int BM = 256, BN = 384, NWAVES = 4;
  constexpr bool PAIRED = KIND != DEVIT_EPI_RESIDUAL_F32;   // column order of the n-tiles, tile_row<PAIRED>()
  constexpr int A_SLOT = BM * BK * 2, B_SLOT = BN * BK * 2, B_RING = 2 * A_SLOT;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;

  const int xcd = blockIdx.x & 7, idx = blockIdx.x >> 3, stride = gridDim.x >> 3;
  int first, last;
  {
    const int q = g.total_tiles >> 3, r = g.total_tiles & 7;
    const int start = xcd * q + min(xcd, r);
    first = start + idx;
    last = start + q + (xcd < r ? 1 : 0);
  }
  if (first >= last) return;
#ifdef DEVIT_GEMMFR_STAMP
  const unsigned long long t_entry = __builtin_amdgcn_s_memtime();
  unsigned long long st_sum[6] = {0, 0, 0, 0, 0, 0};   // tiles, K loop, epilogue, d1 (barrier to barrier), d2 (barrier waits), prologue
#endif

  const unsigned lda64 = (unsigned)g.lda * 64u, ldbs = (unsigned)g.ldb * 128u, kb = (unsigned)g.K * (unsigned)g.ldb * 2u;
  const unsigned lds_base = (unsigned)(size_t)LDS_PTR(smem);
  const unsigned wldsa = lds_base + (unsigned)wave * 8192u, wldsb = lds_base + (unsigned)wave * 12288u;   // (+ the slot's offset)

  // prologue: A stages 0, 1 of the first tile; B stages 0, 1 of the cyclic stream (one n-tile: every tile multiplies by the same B)
  TileRef ct = decode_tile<BM, BN, false, true>(g, first);
#pragma unroll
  for (int st = 0; st < 2; ++st) {
    stage_tile<false, BM, NWAVES, true>(ct.a, g.lda, (ct.kt0 + st) * BK, 0, 0, smem + st * A_SLOT, wave, lane);
    const char* ub = (const char*)(ct.b + (size_t)fr_b_row(st, wave, g.K) * g.ldb);
    const unsigned lds0 = lds_base + (unsigned)(B_RING + st * B_SLOT) + (unsigned)wave * 12288u;
#pragma unroll
    for (int i = 0; i < 12; i += 2)
      dma2_uniform<false>(ub, fr_dma_off_b(g.ldb, wave, lane, i), fr_dma_off_b(g.ldb, wave, lane, i + 1), lds0 + i * 1024u);
  }
  wait_vmcnt<0>();
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
  unsigned acur = 0;                // LDS byte offset of the A slot that holds stage 0 of the tile about to start
  const unsigned wv = (unsigned)wave;
  const unsigned bv2 = (unsigned)fr_b_row(2, wave, g.K) * (unsigned)g.ldb * 2u;
  const unsigned bplo = (unsigned)(uintptr_t)ct.b, bphi = (unsigned)((uintptr_t)ct.b >> 32);
#ifdef DEVIT_GEMMFR_STAMP
  st_sum[5] = __builtin_amdgcn_s_memtime() - t_entry;
#endif

  for (int tile = first; tile < last; tile += stride) {
    const bool has_next = tile + stride < last;
    const TileRef nt = has_next ? decode_tile<BM, BN, false, true>(g, tile + stride) : ct;
    const __bf16* a_ptr = ct.a + (size_t)ct.kt0 * BK;
    const __bf16* a_next = nt.a + (size_t)nt.kt0 * BK;
    const unsigned nk = (unsigned)ct.nk, hasnext = (unsigned)__builtin_amdgcn_readfirstlane(has_next ? 1 : 0);
    const devit_epilogue& ep = g.ep;
    // per-lane constants of the K loop, recomputed per tile from an opaque copy of the lane index (see gemm4_kernel)
    unsigned dsA[4], dsB[8], dmaA[4], dmaB[12];
    {
      int lane_k;
      asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(lane_k));
      const int c = lane_k & 15, gq = lane_k >> 4;
#pragma unroll
      for (int kk = 0; kk < 2; ++kk)
#pragma unroll
        for (int par = 0; par < 2; ++par) {
          const int rowA = wm * 128 + 16 * par + c;
          dsA[kk * 2 + par] = (unsigned)(rowA * 128 + (((kk * 4 + gq) ^ swz_row(rowA)) * 16));
        }
      // read_frag<true, 384, PAIRED>: see b_reads() in tools/gen_gemmfr.py
      const int q4 = (lane_k >> 2) & 3, p = lane_k & 3;
#pragma unroll
      for (int x3 = 0; x3 < 4; ++x3) {
        const unsigned row = (unsigned)((gq * 8 + q4) * (BN * 2) + 64 * (x3 ^ q4));
        if constexpr (PAIRED) {
          dsB[x3] = row + (unsigned)(16 * (p ^ ((gq & 1) << 1)));
          dsB[4 + x3] = 0;
        } else {
#pragma unroll
          for (int jp = 0; jp < 2; ++jp) dsB[2 * x3 + jp] = row + (unsigned)(32 * (jp ^ (gq & 1)) + 16 * (p >> 1) + 8 * (p & 1));
        }
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) dsA[i] += lds_base;      // (the asm adds only the slot offsets: the ring need not start at LDS address 0)
#pragma unroll
      for (int i = 0; i < 8; ++i) dsB[i] += lds_base;
#pragma unroll
      for (int i = 0; i < 4; ++i) dmaA[i] = lane_offset<false, BM, NWAVES>(g.lda, wave, lane_k, i, BM);
#pragma unroll
      for (int i = 0; i < 12; ++i) dmaB[i] = fr_dma_off_b(g.ldb, wave, lane_k, i);
    }
    unsigned t0, t1, t2, t3, t4, t5, t6, t7, t8, t9;
    f32x32 c0, c1, c2, c3;
#ifdef DEVIT_GEMMFR_STAMP
    unsigned d1, d2;
    const unsigned long long ts0 = __builtin_amdgcn_s_memtime();
#define DEVIT_FR_STAMP_OUT , [d1] "=&s"(d1), [d2] "=&s"(d2)
#define DEVIT_FR_ASM(O) DEVIT_GEMMFR_KLOOP_##O##_STAMPED_ASM
#define DEVIT_FR_CLOB(O) DEVIT_GEMMFR_KLOOP_##O##_STAMPED_CLOBBERS
#else
#define DEVIT_FR_STAMP_OUT
#define DEVIT_FR_ASM(O) DEVIT_GEMMFR_KLOOP_##O##_ASM
#define DEVIT_FR_CLOB(O) DEVIT_GEMMFR_KLOOP_##O##_CLOBBERS
#endif
#define DEVIT_FR_STATEMENT(O)                                                                                                   \
    asm volatile(DEVIT_FR_ASM(O)                                                                                                \
                 : [c0] "=&{v[128:159]}"(c0), [c1] "=&{v[160:191]}"(c1), [c2] "=&{v[192:223]}"(c2), [c3] "=&{v[224:255]}"(c3),  \
                   [acur] "+s"(acur), [t0] "=&v"(t0), [t1] "=&v"(t1), [t2] "=&v"(t2), [t3] "=&v"(t3), [t4] "=&v"(t4),           \
                   [t5] "=&v"(t5), [t6] "=&v"(t6), [t7] "=&v"(t7), [t8] "=&v"(t8), [t9] "=&v"(t9) DEVIT_FR_STAMP_OUT            \
                 : [aptr] "s"(a_ptr), [anext] "s"(a_next), [bplo] "s"(bplo), [bphi] "s"(bphi), [bv2] "s"(bv2), [kb] "s"(kb),    \
                   [nk] "s"(nk), [hasnext] "s"(hasnext), [lda64] "s"(lda64), [ldbs] "s"(ldbs), [wldsa] "s"(wldsa),              \
                   [wldsb] "s"(wldsb), [wv] "s"(wv),                                                                            \
                   [dsa0] "v"(dsA[0]), [dsa1] "v"(dsA[1]), [dsa2] "v"(dsA[2]), [dsa3] "v"(dsA[3]),                              \
                   [dsb0] "v"(dsB[0]), [dsb1] "v"(dsB[1]), [dsb2] "v"(dsB[2]), [dsb3] "v"(dsB[3]),                              \
                   [dsb4] "v"(dsB[4]), [dsb5] "v"(dsB[5]), [dsb6] "v"(dsB[6]), [dsb7] "v"(dsB[7]),                              \
                   [dmaa0] "v"(dmaA[0]), [dmaa1] "v"(dmaA[1]), [dmaa2] "v"(dmaA[2]), [dmaa3] "v"(dmaA[3]),                      \
                   [dmab0] "v"(dmaB[0]), [dmab1] "v"(dmaB[1]), [dmab2] "v"(dmaB[2]), [dmab3] "v"(dmaB[3]),                      \
                   [dmab4] "v"(dmaB[4]), [dmab5] "v"(dmaB[5]), [dmab6] "v"(dmaB[6]), [dmab7] "v"(dmaB[7]),                      \
                   [dmab8] "v"(dmaB[8]), [dmab9] "v"(dmaB[9]), [dmab10] "v"(dmaB[10]), [dmab11] "v"(dmaB[11])                   \
                 : DEVIT_FR_CLOB(O))
    if constexpr (PAIRED) DEVIT_FR_STATEMENT(PAIRED);
    else DEVIT_FR_STATEMENT(NATURAL);
#undef DEVIT_FR_STATEMENT
#undef DEVIT_FR_STAMP_OUT
#undef DEVIT_FR_ASM
#undef DEVIT_FR_CLOB
#ifdef DEVIT_GEMMFR_STAMP
    const unsigned long long ts1 = __builtin_amdgcn_s_memtime();
    st_sum[0] += 1; st_sum[1] += ts1 - ts0; st_sum[3] += d1; st_sum[4] += d2;
#endif
    int lane_e;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(lane_e));
    const size_t ob = (size_t)ct.bz * ep.out_batch_stride;
    const int m_lim = ep.m_valid > 0 ? ep.m_valid : g.M;
    if constexpr (KIND == DEVIT_EPI_LNBWD) {
      // ---- fused epilogue: dgrad + LayerNorm backward.  The tile's rows are whole 384-wide rows of exactly the matrix ln_bwd_kernel would read
      // next, so they never go to memory: the accumulators are rounded to bf16 as DEVIT_EPI_STORE_BF16 rounds them and staged in LDS in true
      // column order, 128 rows per pass (m-tiles 4 P .. 4 P + 3 of both wm halves; the ring is dead: this workgroup has no next tile, the host
      // guarantees it), and ln_rows.h's row body runs on them in ln_bwd_kernel's own lane layout -- half a wave per row, the same additions in the
      // same order -- so dx / dx_bf16 are bit for bit what the two launches gave.  The three column sums stay in registers across the tile's 256 rows
      // and leave as partial[tile] (colsum_partials_kernel finishes them: no atomics).  Measured in the serialized step (profiles/r07_a_*): 102 us per
      // launch against 56 (dgrad) + 57 (ln_bwd_kernel) us: the row stage's 273 MB (x, dres, dx, the bf16 copy) cost ~47 us behind the K loop.
      const LnBwdArgs& la = fa.ln;
      const int gq = lane_e >> 4, c = lane_e & 15, hl = lane_e & 31, half = lane_e >> 5;
      f32x4 cs[4];
      float zf;                    // (a zero made here: constants of the epilogue must not live in VGPRs across the K loop, whose statement owns most of them)
      asm volatile("v_mov_b32 %0, 0" : "=v"(zf));
      const f32x4 z4 = {zf, zf, zf, zf};
      LnBwdCols<3> cols;
      ln_bwd_cols_init<3, false>(la, hl, cols, z4);
      float invD = 1.0f / 384.0f;   // (= the standalone kernel's correctly rounded 1.0f / D)
      asm volatile("" : "+v"(invD));
      const size_t zhi = (size_t)__builtin_bit_cast(unsigned, zf) << 32;
      // staged row of (wm, pass-local m-tile pair kk, m-tile u of the pair, row c): wm * 64 + kk * 32 + 16 u + c; columns: the lane's eight at
      // wn * 192 + 64 H + 32 q + 8 gq (tile_row<true>)
      char* const srow = smem + (wm * 64 + c) * LNF_PITCH + (wn * 192 + 8 * gq) * 2;
      // The column group that lives in VGPRs (n-tiles 8..11 of each wn) leaves the registers at once, all four m-tile pairs of it: the second
      // pass's share waits in a side region [128 rows][2 x 64 columns] (nothing of the accumulators stays pinned in VGPRs across the row loop).
      char* const siderow = smem + LNF_SIDE + (wm * 64 + c) * LNF_SIDE_PITCH + (wn * 64 + 8 * gq) * 2;
      auto put_v = [&](const f32x32& cv, int k) {
        int noff[4];
        f32x4 bias[4];
        load_cols<DEVIT_EPI_STORE_BF16>(ep, lane_e, ct.n0 + wn * 192 + 128, noff, bias, cs);
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
          for (int q = 0; q < 2; ++q) {
            float x[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) x[e] = cv[16 * u + 4 * (2 * q + (e >> 2)) + (e & 3)] + bias[2 * q + (e >> 2)][e & 3];
            char* const dst = k < 2 ? srow + ((k & 1) * 32 + 16 * u) * LNF_PITCH + (128 + 32 * q) * 2
                                    : siderow + ((k & 1) * 32 + 16 * u) * LNF_SIDE_PITCH + (32 * q) * 2;
            *(bf16x8*)dst = pack8<false>(x);
          }
      };
      auto put_a = [&](auto hc, auto ic) {
        constexpr int H = decltype(hc)::value, I0 = decltype(ic)::value;
        int noff[4];
        f32x4 bias[4];
        load_cols<DEVIT_EPI_STORE_BF16>(ep, lane_e, ct.n0 + wn * 192 + H * 64, noff, bias, cs);
        f32x4 acc[2][4];
        gemmfr_read_acc<H, I0>(acc);
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
          for (int q = 0; q < 2; ++q) {
            float x[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) x[e] = acc[u][2 * q + (e >> 2)][e & 3] + bias[2 * q + (e >> 2)][e & 3];
            *(bf16x8*)(srow + (((I0 >> 1) & 1) * 32 + 16 * u) * LNF_PITCH + (H * 64 + 32 * q) * 2) = pack8<false>(x);
          }
      };
      // The half-wave's 32 rows of the tile, q = 16 P + t: pass P, staged row t * 8 + (its index among the eight half-waves).  The global inputs of
      // rows q + R .. q + 2 R - 1 are requested before rows q .. q + R - 1 are worked on (the first R before the staging, the second pass's first
      // R across the barriers between the passes): the kernel streams at the rate of its requests in flight.
      constexpr int R = 2;
      struct Pre {
        f32x4 xv[3], dr[3];
        float mu, rs, rsc;
        int m;                                   // the row, -1: a pad row
      };
      auto fetch = [&](int q, Pre& p) {
        const int lr = (q & 15) * 8 + wave * 2 + half;
        const int m = ct.m0 + (lr >> 6) * 128 + 64 * (q >> 4) + (lr & 63);
        const bool live = m < m_lim;
        p.m = live ? m : -1;
        p.rsc = (live && la.dx_bf16 && la.rowscale) ? la.rowscale[(unsigned)m / (unsigned)la.rows_per_scale] : 1.0f;
        p.mu = live ? la.mean[m] : zf;
        p.rs = live ? la.rstd[m] : zf;
#pragma unroll
        for (int v = 0; v < 3; ++v) {
          const size_t o = (zhi | (unsigned)(live ? m : 0)) * 384 + v * 128 + hl * 4;
          p.xv[v] = z4;
          p.dr[v] = z4;
          if (live) {
            p.xv[v] = load_stream((const f32x4*)(la.x + o));
            if (la.dres) p.dr[v] = load_stream((const f32x4*)(la.dres + o));
          }
        }
      };
      Pre cur[R], nxt[R];
      auto ln_pass = [&](int P) {
#pragma unroll 1
        for (int t0 = 0; t0 < LNF_ROWS / 8; t0 += R) {
          if (16 * P + t0 + R < 32) {
#pragma unroll
            for (int i = 0; i < R; ++i) fetch(16 * P + t0 + R + i, nxt[i]);
          }
#pragma unroll
          for (int i = 0; i < R; ++i) {
            const int lr = (t0 + i) * 8 + wave * 2 + half;
            const bool live = cur[i].m >= 0;
            LnBwdRow<3> in;
            in.mu = cur[i].mu;
            in.rs = cur[i].rs;
#pragma unroll
            for (int v = 0; v < 3; ++v) {
              const int col = v * 128 + hl * 4;
              in.xv[v] = cur[i].xv[v];
              in.dyv[v] = z4;
              if (live) {                        // (a pad row's staged line holds what its accumulators held: never read)
                // (second pass: columns 128..191 and 320..383, the VGPR group of wn = 0 / 1, wait in the side region)
                const bool side = P == 1 && ((v == 1 && (col & 127) < 64) || (v == 2 && (col & 127) >= 64));
                const char* src = side ? smem + LNF_SIDE + lr * LNF_SIDE_PITCH + ((v - 1) * 64 + (col & 63)) * 2 : smem + lr * LNF_PITCH + col * 2;
                const bf16x4 t = *(const bf16x4*)src;
                in.dyv[v] = (f32x4){bf2f(t[0]), bf2f(t[1]), bf2f(t[2]), bf2f(t[3])};
              }
            }
            ln_bwd_row<3, false>(la, cols, in, live, zhi | (unsigned)(live ? cur[i].m : 0), lane_e, 384, invD, cur[i].rsc,
                                 [&](int v, size_t) { return cur[i].dr[v]; });
          }
#pragma unroll
          for (int i = 0; i < R; ++i) cur[i] = nxt[i];
        }
      };
      wait_vmcnt<0>();
      __syncthreads();             // every wave's last fragment reads are done: the ring is free
#pragma unroll
      for (int i = 0; i < R; ++i) fetch(i, cur[i]);
      put_v(c0, 0);
      put_v(c1, 1);
      put_v(c2, 2);
      put_v(c3, 3);
      put_a(std::integral_constant<int, 0>(), std::integral_constant<int, 0>());
      put_a(std::integral_constant<int, 1>(), std::integral_constant<int, 0>());
      put_a(std::integral_constant<int, 0>(), std::integral_constant<int, 2>());
      put_a(std::integral_constant<int, 1>(), std::integral_constant<int, 2>());
      __syncthreads();             // both wn waves of every row have written it
      ln_pass(0);
      __syncthreads();             // every half-wave has read its rows: the region is rewritten
      put_a(std::integral_constant<int, 0>(), std::integral_constant<int, 4>());
      put_a(std::integral_constant<int, 1>(), std::integral_constant<int, 4>());
      put_a(std::integral_constant<int, 0>(), std::integral_constant<int, 6>());
      put_a(std::integral_constant<int, 1>(), std::integral_constant<int, 6>());
      __syncthreads();
      ln_pass(1);
      ln_bwd_cols_store<3>(la, cols, (float (*)[3][384])(smem + LNF_RED), wave, lane_e, 384, (size_t)tile);
    } else {
    // epilogue: the eight-wave kernels' register epilogue on chunks of two m-tiles x four n-tiles; the column group that lives in
    // VGPRs (n-tiles 8..11) first -- it frees the registers the other chunks' values are read out into
    const bool full = ct.m0 + BM <= m_lim;
    f32x4 cs[4];   // (no column scale in these kinds)
    auto run = [&](f32x4 (&acc)[2][4], const int (&noff)[4], const f32x4 (&bias)[4], int i0) {
      const int mw = ct.m0 + wm * 128 + i0 * 16;
      if (full) epilogue_direct<KIND, 2, true, false>(ep, acc, noff, bias, cs, lane_e, mw, m_lim, ob);
      else epilogue_direct<KIND, 2, false, false>(ep, acc, noff, bias, cs, lane_e, mw, m_lim, ob);
    };
    {
      int noff[4];
      f32x4 bias[4];
      load_cols<KIND>(ep, lane_e, ct.n0 + wn * 192 + 128, noff, bias, cs);
      auto from_v = [&](const f32x32& c, int i0) {
        f32x4 acc[2][4];
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
          for (int j = 0; j < 4; ++j)
            acc[u][j] = (f32x4){c[16 * u + 4 * j], c[16 * u + 4 * j + 1], c[16 * u + 4 * j + 2], c[16 * u + 4 * j + 3]};
        run(acc, noff, bias, i0);
      };
      from_v(c0, 0);
      from_v(c1, 2);
      from_v(c2, 4);
      from_v(c3, 6);
    }
    auto group = [&](auto hc) {
      constexpr int H = decltype(hc)::value;
      int noff[4];
      f32x4 bias[4];
      load_cols<KIND>(ep, lane_e, ct.n0 + wn * 192 + H * 64, noff, bias, cs);
      auto chunk = [&](auto ic) {
        constexpr int I0 = decltype(ic)::value;
        f32x4 acc[2][4];
        gemmfr_read_acc<H, I0>(acc);
        run(acc, noff, bias, I0);
      };
      chunk(std::integral_constant<int, 0>());
      chunk(std::integral_constant<int, 2>());
      chunk(std::integral_constant<int, 4>());
      chunk(std::integral_constant<int, 6>());
    };
    group(std::integral_constant<int, 0>());
    group(std::integral_constant<int, 1>());
    }
#ifdef DEVIT_GEMMFR_STAMP
    st_sum[2] += __builtin_amdgcn_s_memtime() - ts1;
#endif
    ct = nt;
  }
  wait_vmcnt<0>();   // (requests of a next tile that does not exist are never made; this only drains the epilogue's stores)
#ifdef DEVIT_GEMMFR_STAMP
  if (g.ep.pos && lane == 0) {
    unsigned long long* dbg = (unsigned long long*)g.ep.pos + ((size_t)blockIdx.x * NWAVES + wave) * 8;
#pragma unroll
    for (int q = 0; q < 6; ++q) dbg[q] = st_sum[q];
    dbg[6] = t_entry; dbg[7] = __builtin_amdgcn_s_memtime();
  }
#endif
}

}  // namespace

int devit_gemm::launch_gemmfr(const GemmParams& p, const LnBwdArgs* ln, unsigned grid, hipStream_t s) {
  const GemmArgs g{p};
  constexpr int lds = (256 + 384) * 128 * 2;
  if (ln) return launch_kernel<gemmfr_kernel<DEVIT_EPI_LNBWD>, lds>(grid, 256, s, FrArgs<DEVIT_EPI_LNBWD>{g, *ln});
  if (g.ep.kind == DEVIT_EPI_STORE_BF16) return launch_kernel<gemmfr_kernel<DEVIT_EPI_STORE_BF16>, lds>(grid, 256, s, FrArgs<DEVIT_EPI_STORE_BF16>{g});
  return launch_kernel<gemmfr_kernel<DEVIT_EPI_RESIDUAL_F32>, lds>(grid, 256, s, FrArgs<DEVIT_EPI_RESIDUAL_F32>{g});
}
