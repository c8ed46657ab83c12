// Body of attn_fwd_kernel (ATTN_DROP 0) and attn_fwd_drop_kernel (ATTN_DROP 1): included by csrc/attention.hip, see there.
// Expects from the enclosing kernel: template parameter `F16`, `const AttnFwdArgs a`; with ATTN_DROP 1 also `const DropKey dk`.
#if ATTN_DROP      // the row's 1 / sum carries 1 / (1 - p)
#define ATTN_GATE (gate * dk.s)
#else
#define ATTN_GATE gate
#endif
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* k_img = smem;
  char* v_img = smem + FWD_IMG;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int b = blockIdx.x / a.H, h = blockIdx.x % a.H;
  const int D = a.H * HD, N = a.N, NQ = a.NQ;
  const size_t rs = (size_t)a.q_rs, krs = (size_t)a.kv_rs;
  const __bf16* qbase = a.q + (size_t)b * NQ * rs + h * HD;
  const float c2 = a.scale * 1.4426950408889634f;  // scores in log2 domain
#ifdef DEVIT_ATTN_STAMP    // diagnostic build (tools/attn_stamps.py): head_gate carries a u64 stamp buffer, 8 per workgroup
  unsigned long long* stamps = (unsigned long long*)a.head_gate + (size_t)blockIdx.x * 8;
  const float gate = 1.0f;
  if (tid == 0) { stamps[0] = __builtin_amdgcn_s_memrealtime(); stamps[1] = __builtin_amdgcn_s_memtime(); }
#else
  const float gate = a.head_gate ? a.head_gate[h] : 1.0f;
#endif
  const int ntile = (NQ + 15) >> 4;                  // query tiles
  const int g = lane >> 4, lc = lane & 15;
  const int tq = (lane >> 2) & 3, tp = lane & 3;     // transposed-read row / column-quad of this lane
  constexpr int QT = (MAXT + FWD_WAVES - 1) / FWD_WAVES;   // query tiles per wave
  // Q fragments of ALL this wave's query tiles first, then the K / V images: one exposed HBM latency per workgroup
  // (fetched in MFMA layout, 16 rows x 64 bytes per instruction; whole 128-byte rows + a lane trade afterwards measured 0.04 ms
  // per step SLOWER, profiles/r03_B_attention_rows.txt)
  bf16x8 qall[QT][2];
#pragma unroll
  for (int it = 0; it < QT; ++it) {
    const bf16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
    const int q_ = (wave + it * FWD_WAVES) * 16 + lc;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk)
      qall[it][kk] = (wave + it * FWD_WAVES < ntile && q_ < NQ) ? *(const bf16x8*)(qbase + (size_t)q_ * rs + kk * 32 + g * 8) : z;
  }
  // K and V images by LDS-DMA: no register round trip, no ds_write pass (forward -6 ... -10 % against register staging, same
  // box, profiles/r02_l_attention_dma_prologue.txt); the Q fragments above go straight to registers in MFMA layout
  dma_image<FWD_WAVES, FWD_ROWS>(k_img, a.k + (size_t)b * N * krs + h * HD, krs, N, wave, lane);
  dma_image<FWD_WAVES, FWD_ROWS>(v_img, a.v + (size_t)b * N * krs + h * HD, krs, N, wave, lane);
#ifdef DEVIT_ATTN_STAMP
  if (tid == 0) stamps[6] = __builtin_amdgcn_s_memtime();      // loads issued
#endif
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's share has landed; the barrier covers the others'
#ifdef DEVIT_ATTN_STAMP
  if (tid == 0) stamps[7] = __builtin_amdgcn_s_memtime();      // ... landed (wave 0)
#endif
  __syncthreads();
#ifdef DEVIT_ATTN_STAMP
  if (tid == 0) stamps[2] = __builtin_amdgcn_s_memtime();      // images complete
#endif
  const int tmask = N >> 4;                          // first key tile that contains a key >= N

#pragma unroll
  for (int it = 0; it < QT; ++it) {
    const int qt = wave + it * FWD_WAVES;
    if (qt >= ntile) break;
    const int q = qt * 16 + lc;                      // this lane's query
    f32x4 s[MAXT + 1];
#pragma unroll
    for (int t = 0; t < MAXT; ++t) {
      s[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) s[t] = mfma16t<F16>(img_row_frag(k_img, t * 16, kk, lane), qall[it][kk], s[t]);
    }
    // raw-score row max (scale > 0); only tiles >= tmask can hold padded keys
    float mx = -INFINITY;
#pragma unroll
    for (int t = 0; t < MAXT; ++t) {
      if (t >= tmask) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (t * 16 + g * 4 + r >= N) s[t][r] = -INFINITY;
      }
      mx = fmaxf(fmaxf(fmaxf(s[t][0], s[t][1]), fmaxf(s[t][2], s[t][3])), mx);
    }
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float mxs = mx * c2;
    float sum = 0.f;
#pragma unroll
    for (int t = 0; t < MAXT; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        s[t][r] = __builtin_amdgcn_exp2f(fmaf(s[t][r], c2, -mxs));   // exp2(-inf) = 0 for padded keys
        sum += s[t][r];
      }
    s[MAXT] = (f32x4){0.f, 0.f, 0.f, 0.f};           // keys 208..223
    sum += __shfl_xor(sum, 16, 64);
    sum += __shfl_xor(sum, 32, 64);
    if (a.lse && g == 0 && q < NQ) a.lse[((size_t)b * a.H + h) * NQ + q] = (mxs + log2f(sum)) * 0.6931471805599453f;
#if ATTN_DROP
    {
      // logical tensor: row (b H + h) N + q, column = key, pitch ceil4(N); the head's base is wave-uniform, the rest fits 32 bits
      const unsigned pitch = (N + 3) & ~3;
      const unsigned long long e_row = (unsigned long long)(b * a.H + h) * (unsigned)N * pitch + (unsigned)min(q, NQ - 1) * pitch;
#pragma unroll
      for (int t = 0; t < MAXT; ++t) {
        if (t * 16 < N) {
          const u32x4 w = drop_words(dk, e_row + (unsigned)(t * 16 + g * 4));
#pragma unroll
          for (int r = 0; r < 4; ++r) s[t][r] = w[r] >= dk.thr ? s[t][r] : 0.f;
        }
      }
    }
#endif

    f32x4 o[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) o[dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < 7; ++ks) {
      const f32x4 p0 = s[2 * ks], p1 = s[2 * ks + 1];
      const bf16x8 pf = cvt8<F16>(p0, p1);
      // keys of tile 2ks / 2ks+1 for this lane group; tile 13 (keys 208..223) has P = 0 and, in the 208-row image, no rows:
      // its operand is read from tile 12's rows (any finite values do)
      const int r0 = ks * 32 + g * 4 + tq, r1 = (FWD_ROWS < KROWS && ks == 6) ? r0 : r0 + 16;
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        const int ch = dt * 2 + (tp >> 1), sub = (tp & 1) * 8;
        const bf16x8 vf = cat8(lds_tr_read(v_img + img_off(r0, ch) + sub), lds_tr_read(v_img + img_off(r1, ch) + sub));
        o[dt] = mfma16t<F16>(vf, pf, o[dt]);         // O^T[d][q] += V^T[d][key] P^T[key][q]
      }
    }
#if DEVIT_ATTN_OUT_ROWS
    {
      // Lane (g, lc) holds O[q = lc][d = 16 dt + 4 g + r]: stored from here, an instruction covers 16 rows x 32 bytes -- quarter
      // cache lines, four times the transactions of the bytes (ablation: the output stores cost 10 / 25 us of a 62 / 111 us
      // launch for a quarter of the bytes it reads).  Through this wave's private [16][64] LDS slab instead: two
      // instructions of eight whole 128-byte rows.
      const float sc = ATTN_GATE / sum;
      char* slab = smem + 2 * FWD_IMG + wave * (16 * OSLAB_ROW);
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) *(bf16x4*)(slab + lc * OSLAB_ROW + (dt * 16 + g * 4) * 2) = cvt4<F16>(o[dt] * sc);
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        const int row = half * 8 + (lane >> 3), c8 = lane & 7, qr = qt * 16 + row;
        const bf16x8 v = *(const bf16x8*)(slab + row * OSLAB_ROW + c8 * 16);     // (same wave wrote it: ordered by lgkmcnt)
        if (qr < NQ) *(bf16x8*)(a.out + ((size_t)b * NQ + qr) * D + h * HD + c8 * 8) = v;
      }
    }
#else
    if (q < NQ) {
      const float sc = ATTN_GATE / sum;
      __bf16* orow = a.out + ((size_t)b * NQ + q) * D + h * HD + g * 4;
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        *(bf16x4*)(orow + dt * 16) = cvt4<F16>(o[dt] * sc);
      }
    }
#endif
  }
#ifdef DEVIT_ATTN_STAMP
  if (tid == 0) stamps[3] = __builtin_amdgcn_s_memtime();      // wave 0's compute + store issue done
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if (tid == 0) { stamps[4] = __builtin_amdgcn_s_memtime(); stamps[5] = __builtin_amdgcn_s_memrealtime(); }
#endif
#undef ATTN_GATE
