// Body of attn_bwd4_kernel (ATTN_DROP 0) and attn_bwd4_drop_kernel (ATTN_DROP 1): included by csrc/attention.hip, see there.
// Expects from the enclosing kernel: `const AttnBwdArgs a`; with ATTN_DROP 1 also `const DropKey dkey`.  Defines nothing that outlives it.
#if ATTN_DROP      // x times keep / (1 - p) of (query 4 g + r, this lane's key)
#define ATTN_DROPPED(x, r) ((x) * ((km >> (r)) & 1 ? dkey.s : 0.f))
#else
#define ATTN_DROPPED(x, r) (x)
#endif
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* k_img = smem;
  char* qd = smem + IMG_BYTES;                       // QD_NST stages x {Q block [32][64], dO block [32][64]}
  char* dst = qd + QD_NST * QD_STAGE;                // dS^T of the current block: [224 keys][DST4_STRIDE]
  float* lse2 = (float*)(dst + DST4_BYTES);
  float* delta = lse2 + KROWS;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int b = blockIdx.x / a.H, h = blockIdx.x % a.H;
  const int D = a.H * HD, N = a.N, NQ = a.NQ;
  const size_t rs = (size_t)a.q_rs, krs = (size_t)a.kv_rs;
  const __bf16* qbase = a.q + (size_t)b * NQ * rs + h * HD;
  const __bf16* kbase = a.k + (size_t)b * N * krs + h * HD;
  const __bf16* vbase = a.v + (size_t)b * N * krs + h * HD;
#ifdef DEVIT_ATTN_STAMP    // diagnostic build (tools/attn_stamps.py): head_gate carries a u64 stamp buffer, 8 per workgroup
  unsigned long long* stamps = (unsigned long long*)a.head_gate + (size_t)blockIdx.x * 8;
  const float gate = 1.0f;
  if (tid == 0) { stamps[0] = __builtin_amdgcn_s_memrealtime(); stamps[1] = __builtin_amdgcn_s_memtime(); }
#define ATTN_STAMP(i) do { if (tid == 0) stamps[i] = __builtin_amdgcn_s_memtime(); } while (0)
#else
  const float gate = a.head_gate ? a.head_gate[h] : 1.0f;
#define ATTN_STAMP(i) do { } while (0)
#endif
  const __bf16* dobase = a.dout + (size_t)b * NQ * D + h * HD;
  const __bf16* obase = a.out + (size_t)b * NQ * D + h * HD;
  const int g = lane >> 4, lc = lane & 15;
  const int tq = (lane >> 2) & 3, tp = lane & 3;
  const int ntile = (N + 15) >> 4;
  const int nblk = (NQ + 31) >> 5;

  // ---- prologue: K image and the first Q / dO block by LDS-DMA; V fragments of this wave's key tiles straight to registers;
  // delta[q] = sum_d dO[q][d] O[q][d] and lse from global rows
  dma_image<B4_WAVES>(k_img, kbase, krs, N, wave, lane);
#pragma unroll
  for (int pb = 0; pb < QD_NST - 1; ++pb)
    if (pb < nblk) {
      dma_block(qd + pb * QD_STAGE, qbase, rs, pb * 32, NQ, wave, lane);
      dma_block(qd + pb * QD_STAGE + 32 * HD * 2, dobase, (size_t)D, pb * 32, NQ, wave, lane);
    }
  bf16x8 vf[B4_KT][2];
#pragma unroll
  for (int t = 0; t < B4_KT; ++t) {
    const int key = min((wave + t * B4_WAVES) * 16 + lc, N - 1);
#pragma unroll
#ifdef DEVIT_ATTN_ABL_NOV       // ablation build (round 6): no V loads
    for (int kk = 0; kk < 2; ++kk) asm volatile("" : "=v"(vf[t][kk]));
#else
    for (int kk = 0; kk < 2; ++kk) vf[t][kk] = *(const bf16x8*)(vbase + (size_t)key * krs + kk * 32 + g * 8);
#endif
  }
  {
    constexpr int NT = B4_WAVES * 64;
    RowRegs<NT> dr, orr;
#ifdef DEVIT_ATTN_ABL_NODELTA   // ablation build (round 6): no dO / O rows for delta
#pragma unroll
    for (int it = 0; it < RowRegs<NT>::ITERS; ++it) { asm volatile("" : "=v"(dr.v[it])); asm volatile("" : "=v"(orr.v[it])); }
#else
    fetch_rows(dr, dobase, (size_t)D, NQ, tid);
    fetch_rows(orr, obase, (size_t)D, NQ, tid);
#endif
    ATTN_STAMP(6);                                     // every prologue load is issued
#ifdef DEVIT_ATTN_STAMP
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    ATTN_STAMP(7);                                     // ... and has landed
#endif
    for (int i = tid; i < DST4_BYTES / 16; i += NT) ((f32x4*)dst)[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int it = 0; it < RowRegs<NT>::ITERS; ++it) {
      const int idx = tid + it * NT, row = idx >> 3, c = idx & 7;
      float dl = 0.f;
#pragma unroll
      for (int e = 0; e < 8; ++e) dl += bf2f(dr.v[it][e]) * bf2f(orr.v[it][e]);
      dl += __shfl_xor(dl, 1, 64);
      dl += __shfl_xor(dl, 2, 64);
      dl += __shfl_xor(dl, 4, 64);
      if (c == 0 && row < KROWS) {
        delta[row] = dl * a.scale;                   // pre-scaled: dS = P * (dP * gate * scale - delta * scale)
        lse2[row] = row < NQ ? a.lse[((size_t)b * a.H + h) * NQ + row] * 1.4426950408889634f : 0.f;
      }
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  ATTN_STAMP(2);

  const float c2 = a.scale * 1.4426950408889634f;
  const float gs = gate * a.scale;
  f32x4 dv[B4_KT][4], dk[B4_KT][4];  // [key tile of this wave][d tile]: rows d = 4g + r, col key = lc
#pragma unroll
  for (int i = 0; i < B4_KT; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      dv[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
      dk[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }

#ifdef DEVIT_ATTN_ABL_NOMAIN    // ablation build (round 6): prologue + final stores only
  for (int qb = 0; qb < (a.N < 0 ? nblk : 0); ++qb) {
#else
  for (int qb = 0; qb < nblk; ++qb) {
#endif
    const char* q_blk = qd + (qb & (QD_NST - 1)) * QD_STAGE;
    const char* do_blk = q_blk + 32 * HD * 2;
    // Q / dO of block qb + 3 into the stage block qb - 1 was read from (every wave is past that block's barriers).  Exactly
    // two LDS-DMA instructions per wave and block: the counted wait below relies on it.
    if (qb + QD_NST - 1 < nblk) {
      char* nq = qd + ((qb + QD_NST - 1) & (QD_NST - 1)) * QD_STAGE;
      dma_block(nq, qbase, rs, (qb + QD_NST - 1) * 32, NQ, wave, lane);
      dma_block(nq + 32 * HD * 2, dobase, (size_t)D, (qb + QD_NST - 1) * 32, NQ, wave, lane);
    }
    // ---- per key tile of this wave: S and dP against the block's two query tiles -> P, dS (registers = MFMA operands, dS^T also
    // to LDS), then dV^T += dO^T P and dK^T += Q^T dS.  The block's Q / dO fragments are read from LDS per tile, not held
    // across tiles: with 128 accumulator and 32 V-fragment registers there is no room for them (256 per wave at two
    // workgroups per CU), and LDS has the bandwidth (~70 KB per wave and block).
#pragma unroll
    for (int t = 0; t < B4_KT; ++t) {
      const int kt = wave + t * B4_WAVES;
      if (kt < ntile) {
        asm volatile("" ::: "memory");                 // keep hipcc from hoisting (and keeping alive) the loop-invariant LDS reads
        bf16x8 kf[2];
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) kf[kk] = img_row_frag(k_img, kt * 16, kk, lane);
        f32x4 pp[2], ds[2];
        const bool kok = kt * 16 + lc < N;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
#if ATTN_DROP
          unsigned km = 0;                             // bit r: (query 4 g + r, this lane's key) is kept
          {
            const int p = lane & 3, q0 = qb * 32 + i * 16 + g * 4;
            // logical tensor: row (b H + h) N + q, column = key, pitch ceil4(N); the head's base is wave-uniform, the rest fits 32 bits
            const unsigned pitch = (N + 3) & ~3;
            const unsigned long long e_head = (unsigned long long)(b * a.H + h) * (unsigned)N * pitch;
            const u32x4 w = drop_words(dkey, e_head + ((unsigned)min(q0 + p, NQ - 1) * pitch + (unsigned)(kt * 16 + (lc & ~3))));
            // lane p holds row p's words of keys 0..3 of the quad; it wants word p of rows 0..3: trade with lane p ^ x the word of ITS key
            unsigned got[4];
            got[0] = w[0];
#pragma unroll
            for (int e = 1; e < 4; ++e) got[0] = p == e ? w[e] : got[0];
#pragma unroll
            for (int x = 1; x < 4; ++x) {
              unsigned send = w[x];                    // word p ^ x
#pragma unroll
              for (int e = 1; e < 4; ++e) send = p == e ? w[e ^ x] : send;
              got[x] = x == 1   ? __builtin_amdgcn_update_dpp(0u, send, 0xB1 /* quad_perm [1,0,3,2] */, 0xf, 0xf, false)
                       : x == 2 ? __builtin_amdgcn_update_dpp(0u, send, 0x4E /* quad_perm [2,3,0,1] */, 0xf, 0xf, false)
                                : __builtin_amdgcn_update_dpp(0u, send, 0x1B /* quad_perm [3,2,1,0] */, 0xf, 0xf, false);
            }
            // got[x] = row (p ^ x)'s word of this lane's key
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              unsigned wr = got[r];                    // p == 0
#pragma unroll
              for (int e = 1; e < 4; ++e) wr = p == e ? got[r ^ e] : wr;
              km |= (wr >= dkey.thr ? 1u : 0u) << r;
            }
          }
#endif
          f32x4 sv = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int kk = 0; kk < 2; ++kk) {
            sv = mfma16(img_row_frag(q_blk, i * 16, kk, lane), kf[kk], sv);       // S[q][key], key on the lane
            dp = mfma16(img_row_frag(do_blk, i * 16, kk, lane), vf[t][kk], dp);   // dP[q][key] (before the head gate)
          }
          const f32x4 l2 = *(const f32x4*)(lse2 + qb * 32 + i * 16 + g * 4), dl = *(const f32x4*)(delta + qb * 32 + i * 16 + g * 4);
          // The kernel is bound by vector-instruction issue (~1150 per wave and block before this form), not by MFMA or
          // memory: four instructions per element on the interior (fma, v_exp, fma, mul), the masks only where padded keys
          // (last key tile) or padded queries (last block) exist -- wave-uniform branch.
          if (kt * 16 + 16 <= N && qb * 32 + i * 16 + 16 <= NQ) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const float p = __builtin_amdgcn_exp2f(fmaf(sv[r], c2, -l2[r]));
              pp[i][r] = ATTN_DROPPED(p, r);
              ds[i][r] = p * fmaf(ATTN_DROPPED(dp[r], r), gs, -dl[r]);
            }
          } else {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const bool ok = kok && (qb * 32 + i * 16 + g * 4 + r < NQ);
              const float p = ok ? __builtin_amdgcn_exp2f(fmaf(sv[r], c2, -l2[r])) : 0.f;
              pp[i][r] = ATTN_DROPPED(p, r);
              ds[i][r] = p * fmaf(ATTN_DROPPED(dp[r], r), gs, -dl[r]);
            }
          }
          // dS^T[key][q = 16 i + 4 g + r], 4 consecutive queries = one 8-byte store
          const bf16x4 dsb = {f2bf(ds[i][0]), f2bf(ds[i][1]), f2bf(ds[i][2]), f2bf(ds[i][3])};
          *(bf16x4*)(dst + (kt * 16 + lc) * (DST4_STRIDE * 2) + (i * 16 + g * 4) * 2) = dsb;
        }
        const bf16x8 pf = {f2bf(pp[0][0]), f2bf(pp[0][1]), f2bf(pp[0][2]), f2bf(pp[0][3]),
                           f2bf(pp[1][0]), f2bf(pp[1][1]), f2bf(pp[1][2]), f2bf(pp[1][3])};
        const bf16x8 dsf = {f2bf(ds[0][0]), f2bf(ds[0][1]), f2bf(ds[0][2]), f2bf(ds[0][3]),
                            f2bf(ds[1][0]), f2bf(ds[1][1]), f2bf(ds[1][2]), f2bf(ds[1][3])};
        // A operands dO^T, Q^T: k-slot (g, j) = query 16 (j>>2) + 4g + (j&3), transposed reads of the block images
        const int r0 = g * 4 + tq, r1 = r0 + 16;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
          const int ch = dt * 2 + (tp >> 1), sub = (tp & 1) * 8;
          const bf16x8 dot = cat8(lds_tr_read(do_blk + img_off(r0, ch) + sub), lds_tr_read(do_blk + img_off(r1, ch) + sub));
          const bf16x8 qtt = cat8(lds_tr_read(q_blk + img_off(r0, ch) + sub), lds_tr_read(q_blk + img_off(r1, ch) + sub));
          dv[t][dt] = mfma16(dot, pf, dv[t][dt]);      // dV^T[d][key] += dO^T[d][q] P[q][key]
          dk[t][dt] = mfma16(qtt, dsf, dk[t][dt]);     // dK^T[d][key] += Q^T[d][q] dS[q][key]
        }
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();                       // Y1: dS^T of this block complete
    asm volatile("" ::: "memory");                      // (s_barrier is IntrNoMem: no LDS access may be moved across it)
    // This wave's share of block qb + 1 must have landed before Y2.  vmcnt retires in order; DMA(qb + 1) was issued at the top of
    // iteration qb - 2, and newer than its two instructions are EIGHT operations: the two dq stores of block qb - 2, DMA(qb + 2)
    // x 2, the two dq stores of block qb - 1, DMA(qb + 3) x 2.  vmcnt(6) is therefore stricter than necessary by the two oldest
    // stores (issued two blocks ago: free); do NOT read the 6 as the exact count and trim the wait by it.  All of these exist for
    // every block that has a successor (a block with a successor is full: both of its dq stores are issued by every wave),
    // and without them the wait is only stricter.
    if (qb + 1 < nblk) {
      if (qb + QD_NST - 1 < nblk) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    {
      // dQ^T[d][q] = sum_key K^T[d][key] dS^T[key][q]: wave -> d tile, both query tiles of the block
      f32x4 dq[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
#pragma unroll
      for (int ks = 0; ks < 7; ++ks) {
        const int kr = ks * 32 + g * 8 + tq;
        const bf16x8 kfr = img_tr_frag(k_img, ks * 32, wave * 16, lane);
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          const char* pb = dst + kr * (DST4_STRIDE * 2) + (i * 16 + tp * 4) * 2;
          const bf16x8 bfr = cat8(lds_tr_read(pb), lds_tr_read(pb + 4 * DST4_STRIDE * 2));
          dq[i] = mfma16(kfr, bfr, dq[i]);
        }
      }
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int q = qb * 32 + i * 16 + lc;
        if (q < NQ) {
          const size_t o = ((size_t)b * NQ + q) * a.dq_rs + h * HD + wave * 16 + g * 4;
          store_grad4(a.dq + o, a.dq_add ? a.dq_add + o : nullptr, dq[i]);
        }
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();                       // Y2: dS^T free again; every wave's share of block qb + 1 is in LDS
    asm volatile("" ::: "memory");
  }
  ATTN_STAMP(3);
  // ---- dK, dV of this wave's key tiles through a private fp32 LDS slab: whole 128-byte rows, 16 bytes per lane
  __syncthreads();                                   // every wave has finished reading the images / dS^T
  {
    constexpr int SROW = 272;
    char* slab = smem + wave * (2 * 16 * SROW);
#pragma unroll
    for (int t = 0; t < B4_KT; ++t) {
      const int kt = wave + t * B4_WAVES;
      if (kt >= ntile) break;
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        *(f32x4*)(slab + lc * SROW + (dt * 16 + g * 4) * 4) = dk[t][dt];
        *(f32x4*)(slab + 16 * SROW + lc * SROW + (dt * 16 + g * 4) * 4) = dv[t][dt] * gate;
      }
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        const int row = half * 8 + (lane >> 3), c8 = lane & 7, key = kt * 16 + row;
        if (key < N) {
          const size_t oo = ((size_t)b * N + key) * a.dkv_rs + h * HD + c8 * 8;
#pragma unroll
          for (int which = 0; which < 2; ++which) {            // 0: dK, 1: dV
            const char* src = slab + which * 16 * SROW + row * SROW + c8 * 32;
            f32x4 lo = *(const f32x4*)src, hi = *(const f32x4*)(src + 16);
            const __bf16* add = which ? a.dv_add : a.dk_add;
            if (add) {
              const bf16x8 e = *(const bf16x8*)(add + oo);
              lo += (f32x4){bf2f(e[0]), bf2f(e[1]), bf2f(e[2]), bf2f(e[3])};
              hi += (f32x4){bf2f(e[4]), bf2f(e[5]), bf2f(e[6]), bf2f(e[7])};
            }
            const bf16x8 v = {f2bf(lo[0]), f2bf(lo[1]), f2bf(lo[2]), f2bf(lo[3]), f2bf(hi[0]), f2bf(hi[1]), f2bf(hi[2]), f2bf(hi[3])};
            *(bf16x8*)((which ? a.dv : a.dk) + oo) = v;
          }
        }
      }
    }
  }
#ifdef DEVIT_ATTN_STAMP
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if (tid == 0) { stamps[4] = __builtin_amdgcn_s_memtime(); stamps[5] = __builtin_amdgcn_s_memrealtime(); }
#endif
#undef ATTN_DROPPED
#undef ATTN_STAMP
