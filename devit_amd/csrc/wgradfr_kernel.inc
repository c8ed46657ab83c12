// The body of wgradfr_kernel (wgradfr.hip), included once per instantiation: WGRADFR_KERNEL names it, WGRADFR_DET == 0 is the kernel of the default
// path (partial tiles leave as fp32 atomics), 1 the one of deterministic mode (plain stores into the (slice, tile)'s own place in the workspace).
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1)))
#if WGRADFR_DET
void WGRADFR_KERNEL(const WgDetArgs g) {
#else
void WGRADFR_KERNEL(const WgArgs g) {
#endif
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int BM = 256, BN = 384, NWAVES = 4;
  constexpr int A_SLOT = BM * BK * 2, B_SLOT = BN * BK * 2, B_RING = 2 * A_SLOT;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;

  // workgroups b, b + 8, ... share an XCD: each XCD takes a contiguous run of (slice, tile) pairs, tile fastest -- the tiles of one job and
  // slice (2-6 of them) read the same B rows at the same time through that XCD's L2
  int L;
  {
    const int xcd = blockIdx.x & 7, idx = blockIdx.x >> 3;
    const int q = g.total >> 3, r = g.total & 7;
    if (idx >= q + (xcd < r ? 1 : 0)) return;
    L = xcd * q + min(xcd, r) + idx;
  }
#ifdef DEVIT_GEMMFR_STAMP
  const unsigned long long t_entry = __builtin_amdgcn_s_memtime();
#endif
  const int z = L / g.tiles, t = L - z * g.tiles;
  int ji = 0;
  for (int j = 1; j < g.njobs; ++j)
    if (t >= g.job[j].tile0) ji = j;
  const WgJob& jb = g.job[ji];
  const int m0 = (t - jb.tile0) * BM;
  const int valid = min(BM, jb.a_cols - m0);                    // 256 or 128 columns of A exist in this tile
  const int kt0 = (int)((long long)z * g.nk_total / g.split);
  const int nk_i = (int)((long long)(z + 1) * g.nk_total / g.split) - kt0;
  const int lda = jb.lda, ldb = jb.ldb;
  const __bf16* a_tile = jb.a + (size_t)kt0 * BK * lda + m0;    // &A[k0][m0]
  const __bf16* b_sl = jb.b + (size_t)kt0 * BK * ldb;           // &B[k0][0]
  const int Ks = nk_i * BK;                                     // the slice: B's half-stage-shifted stream is cyclic in it

  const unsigned ldas = (unsigned)lda * 128u, ldbs = (unsigned)ldb * 128u, kb = (unsigned)Ks * (unsigned)ldb * 2u;
  const unsigned lds_base = (unsigned)(size_t)LDS_PTR(smem);
  const unsigned wldsa = lds_base + (unsigned)wave * 8192u, wldsb = lds_base + (unsigned)wave * 12288u;

  // prologue: stages 0, 1 of both operands
#pragma unroll
  for (int st = 0; st < 2; ++st) {
    stage_tile<true, BM, NWAVES, true>(a_tile, lda, st * BK, 0, 0, smem + st * A_SLOT, wave, lane, valid);
    const char* ub = (const char*)(b_sl + (size_t)fr_b_row(st, wave, Ks) * ldb);
    const unsigned lds0 = lds_base + (unsigned)(B_RING + st * B_SLOT) + (unsigned)wave * 12288u;
#pragma unroll
    for (int i = 0; i < 12; i += 2)
      dma2_uniform<false>(ub, fr_dma_off_b(ldb, wave, lane, i), fr_dma_off_b(ldb, wave, lane, i + 1), lds0 + i * 1024u);
  }
  wait_vmcnt<0>();
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
#ifdef DEVIT_GEMMFR_STAMP
  const unsigned long long t_primed = __builtin_amdgcn_s_memtime();
#endif
  unsigned acur = 0;
  const unsigned wv = (unsigned)wave, nk = (unsigned)nk_i;
  const unsigned bv2 = (unsigned)fr_b_row(2, wave, Ks) * (unsigned)ldb * 2u;
  const unsigned bplo = (unsigned)(uintptr_t)b_sl, bphi = (unsigned)((uintptr_t)b_sl >> 32);
  const unsigned ones = jb.colsum ? 0x3f803f80u : 0u;

  // per-lane constants of the K loop (gen_gemmfr.py, KMA variant)
  unsigned dsA[4], dsB[4], dmaA[8], dmaB[12];
  {
    int lane_k;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(lane_k));
    const int gq = lane_k >> 4, q4 = (lane_k >> 2) & 3, p = lane_k & 3;
#pragma unroll
    for (int x = 0; x < 4; ++x) {
      dsA[x] = lds_base + (unsigned)((gq * 8 + q4) * (BM * 2) + 256 * wm + 64 * (x ^ q4) + 16 * (p ^ ((gq & 1) << 1)));
      dsB[x] = lds_base + (unsigned)((gq * 8 + q4) * (BN * 2) + 64 * (x ^ q4) + 16 * (p ^ ((gq & 1) << 1)));
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) dmaA[i] = lane_offset<true, BM, NWAVES>(lda, wave, lane_k, i, valid);
#pragma unroll
    for (int i = 0; i < 12; ++i) dmaB[i] = fr_dma_off_b(ldb, wave, lane_k, i);
  }
  unsigned t0, t1, t2, t3, t4, t5, t6, t7;
  float rs0 = 0.f, rs1 = 0.f, rs2 = 0.f, rs3 = 0.f;
  f32x32 c0, c1, c2, c3;
#ifdef DEVIT_GEMMFR_STAMP
  unsigned d1, d2;
  const unsigned long long ts0 = __builtin_amdgcn_s_memtime();
#define DEVIT_WG_STAMP_OUT , [d1] "=&s"(d1), [d2] "=&s"(d2)
#define DEVIT_WG_ASM DEVIT_WGRADFR_KLOOP_STAMPED_ASM
#define DEVIT_WG_CLOB DEVIT_WGRADFR_KLOOP_STAMPED_CLOBBERS
#else
#define DEVIT_WG_STAMP_OUT
#define DEVIT_WG_ASM DEVIT_WGRADFR_KLOOP_ASM
#define DEVIT_WG_CLOB DEVIT_WGRADFR_KLOOP_CLOBBERS
#endif
  asm volatile(DEVIT_WG_ASM
               : [c0] "=&{v[128:159]}"(c0), [c1] "=&{v[160:191]}"(c1), [c2] "=&{v[192:223]}"(c2), [c3] "=&{v[224:255]}"(c3),
                 [acur] "+s"(acur), [t0] "=&v"(t0), [t1] "=&v"(t1), [t2] "=&v"(t2), [t3] "=&v"(t3), [t4] "=&v"(t4),
                 [t5] "=&v"(t5), [t6] "=&v"(t6), [t7] "=&v"(t7), [rs0] "+v"(rs0), [rs1] "+v"(rs1), [rs2] "+v"(rs2), [rs3] "+v"(rs3) DEVIT_WG_STAMP_OUT
               : [aptr] "s"(a_tile), [bplo] "s"(bplo), [bphi] "s"(bphi), [bv2] "s"(bv2), [kb] "s"(kb), [nk] "s"(nk), [ldas] "s"(ldas),
                 [ldbs] "s"(ldbs), [wldsa] "s"(wldsa), [wldsb] "s"(wldsb), [wv] "s"(wv), [ones] "s"(ones),
                 [dsa0] "v"(dsA[0]), [dsa1] "v"(dsA[1]), [dsa2] "v"(dsA[2]), [dsa3] "v"(dsA[3]),
                 [dsb0] "v"(dsB[0]), [dsb1] "v"(dsB[1]), [dsb2] "v"(dsB[2]), [dsb3] "v"(dsB[3]),
                 [dmaa0] "v"(dmaA[0]), [dmaa1] "v"(dmaA[1]), [dmaa2] "v"(dmaA[2]), [dmaa3] "v"(dmaA[3]),
                 [dmaa4] "v"(dmaA[4]), [dmaa5] "v"(dmaA[5]), [dmaa6] "v"(dmaA[6]), [dmaa7] "v"(dmaA[7]),
                 [dmab0] "v"(dmaB[0]), [dmab1] "v"(dmaB[1]), [dmab2] "v"(dmaB[2]), [dmab3] "v"(dmaB[3]),
                 [dmab4] "v"(dmaB[4]), [dmab5] "v"(dmaB[5]), [dmab6] "v"(dmaB[6]), [dmab7] "v"(dmaB[7]),
                 [dmab8] "v"(dmaB[8]), [dmab9] "v"(dmaB[9]), [dmab10] "v"(dmaB[10]), [dmab11] "v"(dmaB[11])
               : DEVIT_WG_CLOB);
#undef DEVIT_WG_STAMP_OUT
#undef DEVIT_WG_ASM
#undef DEVIT_WG_CLOB
#ifdef DEVIT_GEMMFR_STAMP
  const unsigned long long ts1 = __builtin_amdgcn_s_memtime();
#endif
  // ---- epilogue.  Lane (g, c) holds, for A tile i and B tile q, register r:  C[row(i, c)][col(q, 4 g + r)] with the PAIRED tile-row order on
  // both sides: row(i, c) = 32 (i >> 1) + 8 (c >> 2) + 4 (i & 1) + (c & 3) of the wave's 128, col(q, .) = 32 (q >> 1) + 8 g + 4 (q & 1) + r of
  // its 192.  Pass k stages the A tiles (2 k, 2 k + 1) = rows 32 k .. 32 k + 31 as [32][192 (+4)] floats in the wave's own LDS region
  // (the ring is free: the K loop's last requests were waited for in its last step) and adds them to `out` a whole row piece per instruction.
  __syncthreads();             // every wave's last fragment reads are done
  int lane_e;
  asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(lane_e));
  constexpr int PITCH = 196;
  float* cw = (float*)smem + wave * (32 * PITCH);
  const int gq = lane_e >> 4, c = lane_e & 15;
  const bool wave_valid = wm * 128 < valid;                  // (a half tile: the rows of the wm = 1 waves do not exist)
  float* wrow = cw + (8 * (c >> 2) + (c & 3)) * PITCH + 8 * gq;
  auto stage = [&](const f32x4 (&acc)[2][4], int H) {       // n-tiles 4 H .. 4 H + 3 of A tiles (2 k, 2 k + 1)
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int j = 0; j < 4; ++j) *(f32x4*)(wrow + 4 * u * PITCH + 32 * ((4 * H + j) >> 1) + 4 * (j & 1)) = acc[u][j];
  };
  auto flush = [&](int k) {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    const int mb = m0 + wm * 128 + 32 * k;                   // first output row (= A column) of the pass
#if WGRADFR_DET
    // the (slice, tile)'s partial in the tile's own orientation, [256 A columns][384], whatever the job's: the fold launch transposes
    {
      float* o = g.ws + ((size_t)L * BM + wm * 128 + 32 * k) * BN + wn * 192 + lane_e;
#pragma unroll 4
      for (int row = 0; row < 32; ++row) {
        const float* src = cw + row * PITCH + lane_e;
        const float v0 = src[0], v1 = src[64], v2 = src[128];
        float* d = o + (size_t)row * BN;
        d[0] = v0;
        d[64] = v1;
        d[128] = v2;
      }
    }
#else
    if (!jb.transposed) {
      float* o = jb.out + (size_t)mb * jb.ldc + wn * 192 + lane_e;
#pragma unroll 4
      for (int row = 0; row < 32; ++row) {
        const float* src = cw + row * PITCH + lane_e;
        const float v0 = src[0], v1 = src[64], v2 = src[128];
        float* d = o + (size_t)row * jb.ldc;
        unsafeAtomicAdd(d, v0);
        unsafeAtomicAdd(d + 64, v1);
        unsafeAtomicAdd(d + 128, v2);
      }
    } else {
      const int row = lane_e & 31, nsub = lane_e >> 5;
      float* o = jb.out + (size_t)(wn * 192 + nsub) * jb.ldc + mb + row;
      const float* src = cw + row * PITCH + nsub;
#pragma unroll 4
      for (int n2 = 0; n2 < 96; ++n2) unsafeAtomicAdd(o + (size_t)(2 * n2) * jb.ldc, src[2 * n2]);
    }
#endif
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");       // (the region is rewritten by the next pass)
  };
  auto from_v = [&](const f32x32& cv) {
    f32x4 acc[2][4];
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        acc[u][j] = (f32x4){cv[16 * u + 4 * j], cv[16 * u + 4 * j + 1], cv[16 * u + 4 * j + 2], cv[16 * u + 4 * j + 3]};
    stage(acc, 2);
  };
  auto pass = [&](auto kc, const f32x32& cv) {
    constexpr int k = decltype(kc)::value;
    if (wave_valid) {
      from_v(cv);
      f32x4 acc[2][4];
      gemmfr_read_acc<0, 2 * k>(acc);
      stage(acc, 0);
      gemmfr_read_acc<1, 2 * k>(acc);
      stage(acc, 1);
      flush(k);
    }
  };
  pass(std::integral_constant<int, 0>(), c0);
  pass(std::integral_constant<int, 1>(), c1);
  pass(std::integral_constant<int, 2>(), c2);
  pass(std::integral_constant<int, 3>(), c3);
  if (jb.colsum && wave_valid) {
    // lane (G, c) holds the sum over ITS k (8 G .. 8 G + 7 of every 32) of tile row c of A tile 2 x + wn: fold the four G
    float rs[4] = {rs0, rs1, rs2, rs3};
#pragma unroll
    for (int x = 0; x < 4; ++x) {
      float v = rs[x];
      v += __shfl_xor(v, 16, 64);
      v += __shfl_xor(v, 32, 64);
      const int i = 2 * x + wn;
      const int row = wm * 128 + 32 * (i >> 1) + 8 * (c >> 2) + 4 * (i & 1) + (c & 3);
#if WGRADFR_DET
      if (lane_e < 16) g.ws[(size_t)g.total * (BM * BN) + (size_t)L * BM + row] = v;     // behind the tiles: [slice][tile][256] column sums
#else
      if (lane_e < 16) unsafeAtomicAdd(jb.colsum + m0 + row, v);
#endif
    }
  }
#ifdef DEVIT_GEMMFR_STAMP
  if (g.dbg && lane == 0) {      // per wave: K-steps, prologue, K loop, phase sum, barrier-wait sum, epilogue, entry, exit
    unsigned long long* dbg = g.dbg + ((size_t)blockIdx.x * NWAVES + wave) * 8;
    const unsigned long long t_exit = __builtin_amdgcn_s_memtime();
    dbg[0] = nk; dbg[1] = t_primed - t_entry; dbg[2] = ts1 - ts0; dbg[3] = d1; dbg[4] = d2; dbg[5] = t_exit - ts1; dbg[6] = t_entry; dbg[7] = t_exit;
  }
#endif
}
