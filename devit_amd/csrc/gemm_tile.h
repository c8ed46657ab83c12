// gemm_kernel: the eight-wave persistent GEMM on 128x128 tiles (one barrier per K-step) or 256x256 tiles (ping-pong schedule), and the function
// that launches its instantiations of one tile size.  Two units hold them: gemm_tile128.hip and gemm_tile256.hip.
#pragma once
#include "gemm_device.h"

namespace {

// acc + sum of the eight bf16 values of one MFMA fragment (four v_dot2c_f32_bf16 against packed ones)
__device__ __forceinline__ float sum8_bf16(bf16x8 v, float acc) {
  typedef __bf16 bf16x2v __attribute__((ext_vector_type(2)));
  const bf16x2v one = {(__bf16)1.0f, (__bf16)1.0f};
  acc = __builtin_amdgcn_fdot2_f32_bf16(__builtin_shufflevector(v, v, 0, 1), one, acc, false);
  acc = __builtin_amdgcn_fdot2_f32_bf16(__builtin_shufflevector(v, v, 2, 3), one, acc, false);
  acc = __builtin_amdgcn_fdot2_f32_bf16(__builtin_shufflevector(v, v, 4, 5), one, acc, false);
  acc = __builtin_amdgcn_fdot2_f32_bf16(__builtin_shufflevector(v, v, 6, 7), one, acc, false);
  return acc;
}

// Persistent BM x BN x 64 GEMM: WAVES_M x WAVES_N waves (each (BM/WAVES_M) x (BN/WAVES_N)), LDS ring (3 A + 2 B slots)
// filled by LDS-DMA.  A workgroup walks its share of the output tiles and treats their K-steps as ONE stream of ring
// stages: the refill issued during the last K-steps of a tile already belongs to the next tile, so neither the
// DMA latency of a tile's first stages nor the register-only epilogue leaves the ring empty.  One raw barrier per
// K-step (128x128) or the four-interval ping-pong schedule below (256x256).
// Tile order: workgroups b, b+8, ... share an XCD (and its L2); each XCD owns a contiguous run of tiles (n-tile
// fastest inside an L2-sized chunk of B, see decode_tile) and its workgroups walk that run side by side.
template <int BM, int BN, int WAVES_M, int WAVES_N, int NSTAGE, bool A_KM, bool B_KM, int KIND, bool F16 = false>
__global__ __launch_bounds__(WAVES_M * WAVES_N * 64) __attribute__((amdgpu_waves_per_eu(2, 2)))
void gemm_kernel(const GemmArgs g) {
  // the split-K kinds: partial sums leave by fp32 atomics (ATOMIC_F32), or -- deterministic mode, gemm.hip -- by plain stores into the (batch, slice)'s
  // own slab of a workspace that a fold launch adds to the destination in slice order (DET_F32: same K loop, another epilogue, its own instantiation)
  constexpr bool SPLITK = KIND == DEVIT_EPI_ATOMIC_F32 || KIND == devit_gemm::DEVIT_EPI_DET_F32;
  static_assert(!F16 || (KIND != DEVIT_EPI_DGELU_BF16 && !SPLITK && !A_KM && !B_KM),
                "f16 operands: forward layouts / epilogues only (the frozen teacher has no backward)");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int NWAVES = WAVES_M * WAVES_N;
  constexpr int WM = BM / WAVES_M, WN = BN / WAVES_N, MI = WM / 16, NI = WN / 16;
  static_assert(WN == 64 && WM % 64 == 0, "wave tile must be (64 k) x 64");
  static_assert(NSTAGE == 2, "NSTAGE is the B ring depth; uniformly deeper rings at one workgroup per CU lost everywhere");
  // Every epilogue but the split-K atomic one runs straight from the accumulators: the MFMAs then take the B operand
  // (output columns) on their row side, see epilogue_direct().  The atomic one stages through the ring's LDS, so its
  // stream stops at every tile end.
  constexpr bool DIRECT = !SPLITK;
  constexpr bool PAIRED = KIND == DEVIT_EPI_STORE_BF16 || KIND == DEVIT_EPI_GELU_BF16 || KIND == DEVIT_EPI_DGELU_BF16;
  constexpr int A_TILE_BYTES = BM * BK * 2, B_TILE_BYTES = BN * BK * 2;
  // Ring: two B slots, THREE A slots.  A is the operand that streams from HBM (an activation; B is a weight that lives in
  // L2 -- or, in the weight-gradient GEMMs, the narrower activation), so its stages are requested one K-step earlier:
  // two A stages in flight per workgroup at unchanged occupancy (128x128: 2 x 80 KB, 256x256: 160 KB = the whole LDS).
  // Cold-HBM operands: +4...12 % on the 128x128 shapes (tools/gemm_bench.py COLD=1), -1...3 % on cache-resident ones.
  constexpr bool PP = DIRECT && BM == 256 && BN == 256 && WAVES_M == 2;   // ping-pong schedule, below
  constexpr int NA = 3;                                          // A slots (B has 2)
  constexpr int PER_A = (BM / 8) / NWAVES;                       // LDS-DMA instructions per wave per A stage
  constexpr int B_RING = NA * A_TILE_BYTES;                      // LDS offset of the B slots
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WAVES_N, wn = wave % WAVES_N;
#ifdef DEVIT_GEMM_TSTAMP
  const unsigned long long t_entry = __builtin_amdgcn_s_memtime(), rt_entry = __builtin_amdgcn_s_memrealtime();
#endif

  // this workgroup's tiles: first, first + stride, ... < last
  const int xcd = blockIdx.x & 7, idx = blockIdx.x >> 3, stride = gridDim.x >> 3;
  int first, last;
  {
    const int q = g.total_tiles >> 3, r = g.total_tiles & 7;
    const int start = xcd * q + min(xcd, r);
    first = start + idx;
    last = start + q + (xcd < r ? 1 : 0);
  }
  if (first >= last) return;

  // producer cursors: the next B stage to request (p) and, on the 3-slot A ring, the next A stage (q = p + 1 stage)
  struct Cursor {
    TileRef ref;
    int tile, t;
    bool open;
  };
  Cursor pb{decode_tile<BM, BN, A_KM, B_KM>(g, first), first, 0, true};
  Cursor pa = pb;
  int a_slot = 0, b_slot = 0;
  bool a_last = false;   // the newest vector-memory operations of this wave are the PER_A DMAs of an A stage
  auto step_cursor = [&](Cursor& c) {
    if (++c.t == c.ref.nk) {
      c.t = 0;
      c.tile += stride;
      if (DIRECT && c.tile < last) c.ref = decode_tile<BM, BN, A_KM, B_KM>(g, c.tile);
      else c.open = false;
    }
  };
  auto dma_a = [&](const Cursor& c) {
#ifdef DEVIT_GEMM_NODMA       // diagnostic build: MFMAs + LDS reads alone (operands are whatever the LDS holds)
    if (g.K < 0)
#endif
    stage_tile<A_KM, BM, NWAVES>(c.ref.a, g.lda, (c.ref.kt0 + c.t) * BK, g.a_group, g.a_skip,
                                           smem + a_slot * A_TILE_BYTES, wave, lane);
    a_slot = a_slot + 1 == NA ? 0 : a_slot + 1;
  };
  auto dma_b = [&](const Cursor& c) {
#ifdef DEVIT_GEMM_NODMA
    if (g.K < 0)
#endif
    stage_tile<B_KM, BN, NWAVES>(c.ref.b, g.ldb, (c.ref.kt0 + c.t) * BK, g.b_group, g.b_skip,
                                           smem + B_RING + b_slot * B_TILE_BYTES, wave, lane, min(BN, g.N - c.ref.n0));
    b_slot ^= 1;
  };
  auto issue_a = [&]() {
    a_last = pa.open;
    if (!pa.open) return;
    dma_a(pa);
    step_cursor(pa);
  };
  // One refill: B of the next stage first, then A of the stage after it.  The A request is the newest thing in the queue, so "everything but PER_A operations has completed"
  // (wait_stage) means: the stage about to be read has landed, the A stage after it may still be in flight.
  auto produce = [&]() {
    if (pb.open) {
      dma_b(pb);
      step_cursor(pb);
    }
    issue_a();
  };
  auto wait_stage = [&]() {
    if (a_last) wait_vmcnt<PER_A>();
    else wait_vmcnt<0>();
  };
  // ---------------------------------------------------------------------------------------------------------------
  // Ping-pong schedule (256x256 tile: the two waves of a SIMD are wm = 0 and wm = 1 of the SAME workgroup).  With one
  // barrier per K-step all eight waves read their fragments at the same time (96 KB through the LDS while every MFMA
  // pipe idles) and then all issue MFMAs at the same time: SQ_VALU_MFMA_BUSY_CYCLES showed the pipes 51 % busy with
  // the DMA removed.  Here a K-step is four barrier intervals -- reads(kk=0) | MFMA(0) | reads(1) | MFMA(1) -- and the
  // wm = 1 waves run ONE interval behind the wm = 0 waves (one extra barrier before a tile's first K-step, one extra
  // for wm = 0 after its last): in every interval one wave of each SIMD issues its 32 MFMAs while the other reads its next fragments.
  //   interval a: ds_read fragments kk = 0, request B of stage t+1 (the slot read in step t-1), lgkmcnt(0)
  //   interval b: MFMA kk = 0
  //   interval c: ds_read fragments kk = 1, request A of stage t+2, counted vmcnt (this wave's share of stage t+1 has landed), lgkmcnt(0)
  //   interval d: MFMA kk = 1
  // RAW: a wave reads stage t+1 after its barrier Y1(t); the lagging group passed its own vmcnt(0) before its X1(t),
  // which is the same barrier event.  WAR: stage t+1's slot was last read in interval c of step t-1, retired by the
  // lgkmcnt(0) in front of X1(t-1), at least one barrier event before any wave requests stage t+1.
  if constexpr (PP) {
    auto fence = [&]() {
      asm volatile("" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
    };
    auto bar = [&]() {
      fence();
      __builtin_amdgcn_s_barrier();
      fence();
    };
    issue_a();                         // A of stage 0, then B of stage 0 and A of stage 1
    produce();
    wait_vmcnt<0>();
    bar();
    int ca_slot = 0, cb_slot = 0;
#ifdef DEVIT_GEMM_TSTAMP   // diagnostic build: per tile {K loop start, K loop end, epilogue end}, per K-step end of the 2nd tile
    unsigned long long* tdbg = g.ep.pos ? (unsigned long long*)g.ep.pos + ((size_t)blockIdx.x * NWAVES + wave) * 48 : nullptr;
    int tcount = 0;
    if (tdbg && lane == 0) {
      tdbg[40] = t_entry;
      tdbg[42] = rt_entry;
      tdbg[44] = __builtin_amdgcn_s_memtime();      // ring primed: first K loop can start
    }
#endif
    for (int tile = first; tile < last; tile += stride) {
      const TileRef ct = decode_tile<BM, BN, A_KM, B_KM>(g, tile);
      f32x4 acc[MI][NI];
#pragma unroll
      for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
      const devit_epilogue& ep = g.ep;
      const int nw = ct.n0 + wn * WN;
#ifdef DEVIT_GEMM_TSTAMP
      if (tdbg && lane == 0 && tcount < 8) tdbg[tcount * 3 + 0] = __builtin_amdgcn_s_memtime();
#endif
      int noff[4];
      f32x4 bias[4], cs[4];
#ifdef DEVIT_GEMM_STAMP    // diagnostic build: s_memtime at the edges of the four intervals of K-step 3 of the first tile
      unsigned long long stamp[12];
#pragma unroll
      for (int q = 0; q < 12; ++q) stamp[q] = 0;
#define DEVIT_STAMP(q) do { if (t == 3 && tile == first) stamp[q] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define DEVIT_STAMP(q) do { } while (0)
#endif
      if (wm == 1) bar();              // the offset: this group now runs one interval behind
      for (int t = 0; t < ct.nk; ++t) {
        const char* cur_a = smem + ca_slot * A_TILE_BYTES;
        const char* cur_b = smem + B_RING + cb_slot * B_TILE_BYTES;
        ca_slot = ca_slot + 1 == NA ? 0 : ca_slot + 1;
        cb_slot ^= 1;
        if (t == ct.nk - 1 && nw < g.N) load_cols<KIND>(ep, lane, nw, noff, bias, cs);   // under the last K-step
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
          bf16x8 af[MI], bfr[NI];
#ifdef DEVIT_GEMM_NOREAD     // diagnostic build: no fragment reads (operands are whatever the registers hold)
#pragma unroll
          for (int j = 0; j < NI; ++j) asm volatile("" : "=v"(bfr[j]));
#pragma unroll
          for (int i = 0; i < MI; ++i) asm volatile("" : "=v"(af[i]));
#else
#pragma unroll
          for (int j = 0; j < NI; ++j) bfr[j] = read_frag<B_KM, BN, PAIRED>(cur_b, wn * WN, j, kk, lane);
#pragma unroll
          for (int i = 0; i < MI; ++i) af[i] = read_frag<A_KM, BM, false>(cur_a, wm * WM, i, kk, lane);
#endif
          DEVIT_STAMP(kk * 6 + 0);     // fragment reads issued
          // The stage's eight LDS-DMA instructions per wave split over the two read intervals (all eight in the first one
          // made it ~1050 cycles against the partner's 560 cycles of MFMAs; in-kernel stamps, tools/gemm_stamps.py): B of
          // stage t+1 behind the kk = 0 reads, A of stage t+2 behind the kk = 1 reads, then the counted wait (everything
          // but that A request has landed -> stage t+1 readable after the next barrier).  Two other placements lost and are in the git
          // history: the whole refill in front of the kk = 0 reads, and the eight instructions dealt over all four intervals (measured: -10 %).
          fence();
          if (kk == 0) {
            if (pb.open) {
              dma_b(pb);
              step_cursor(pb);
            }
          } else {
            issue_a();
            wait_stage();
          }
          fence();
          DEVIT_STAMP(kk * 6 + 1);     // DMA wait over
          asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
          DEVIT_STAMP(kk * 6 + 2);     // fragments in registers
          bar();
          DEVIT_STAMP(kk * 6 + 3);     // through the barrier
#ifdef DEVIT_GEMM_NOMFMA     // diagnostic build: fragment reads and barriers alone
#pragma unroll
          for (int j = 0; j < NI; ++j) asm volatile("" ::"v"(bfr[j]));
#pragma unroll
          for (int i = 0; i < MI; ++i) asm volatile("" ::"v"(af[i]));
#else
#pragma unroll
          for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int j = 0; j < NI; ++j) acc[i][j] = mfma16t<F16>(bfr[j], af[i], acc[i][j]);
#endif
          DEVIT_STAMP(kk * 6 + 4);     // MFMAs issued
          bar();
          DEVIT_STAMP(kk * 6 + 5);     // through the barrier
        }
#ifdef DEVIT_GEMM_TSTAMP
        if (tdbg && lane == 0 && tcount == 1 && t < 16 && (g.M & 1)) tdbg[24 + t] = __builtin_amdgcn_s_memtime();
#endif
      }
#ifdef DEVIT_GEMM_TSTAMP
      if (tdbg && lane == 0 && tcount < 8) tdbg[tcount * 3 + 1] = __builtin_amdgcn_s_memtime();
#endif
      if (wm == 0) bar();              // pairs with the lagging group's last barrier: both groups run the epilogue
#ifdef DEVIT_GEMM_STAMP
      if (tile == first && lane == 0 && g.ep.pos != nullptr) {
        unsigned long long* dbg = (unsigned long long*)g.ep.pos + ((size_t)blockIdx.x * NWAVES + wave) * 12;
#pragma unroll
        for (int q = 0; q < 12; ++q) dbg[q] = stamp[q];
      }
#endif
      if (nw < g.N) {                  // (a wave whose 64 columns lie past a ragged N has nothing to store)
        settle_cols<KIND>(bias, cs);   // together (one after the other would double its MFMA-idle time)
        const size_t ob = (size_t)ct.bz * ep.out_batch_stride;
        const int m_lim = ep.m_valid > 0 ? ep.m_valid : g.M;
        if (ct.m0 + BM <= m_lim) epilogue_direct<KIND, MI, true, F16>(ep, acc, noff, bias, cs, lane, ct.m0 + wm * WM, m_lim, ob);
        else epilogue_direct<KIND, MI, false, F16>(ep, acc, noff, bias, cs, lane, ct.m0 + wm * WM, m_lim, ob);
      }
#ifdef DEVIT_GEMM_TSTAMP
      if (tdbg && lane == 0 && tcount < 8) tdbg[tcount * 3 + 2] = __builtin_amdgcn_s_memtime();
      ++tcount;
#endif
    }
#ifdef DEVIT_GEMM_TSTAMP
    if (tdbg && lane == 0) {
      tdbg[41] = __builtin_amdgcn_s_memtime();
      tdbg[43] = __builtin_amdgcn_s_memrealtime();
      tdbg[45] = tcount;
    }
#endif
    return;
  }

  issue_a();   // A of the first stage, then B of the first stage and A of the second
  produce();

  // Make the next stage readable: it must have landed, every wave must know so and must have finished reading the
  // slots the refill overwrites (the ones read a step ago).
  auto advance = [&]() {
    wait_stage();
    __builtin_amdgcn_s_barrier();
    produce();
  };

  int ca_slot = 0, cb_slot = 0;
  bool primed = false;   // the stage at c_slot is already readable (advance() ran for it before the last epilogue)
  for (int tile = first; tile < last; tile += stride) {
    const TileRef ct = decode_tile<BM, BN, A_KM, B_KM>(g, tile);
    f32x4 acc[MI][NI];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
      for (int j = 0; j < NI; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    // Split-K weight gradient: the row sums of A (= dY^T, i.e. the bias gradient) come from the fragments the MFMAs
    // read anyway -- one v_dot2c_f32_bf16 per two elements, on the waves that own the first 64 columns of their tile.
    // The n-tiles of one (m-tile, k-slice) see the same A rows, so they share the work: tile tn takes the K-steps
    // kt with kt % tiles_n == tn (every A element is added exactly once).
    float rsum[MI];
#pragma unroll
    for (int i = 0; i < MI; ++i) rsum[i] = 0.f;
    const bool rowsum_on = SPLITK && g.ep.aux != nullptr && wn == 0;
    int rs_wait = 0;          // K-steps until this tile's next turn
    if (rowsum_on) rs_wait = (ct.n0 / BN - ct.kt0 % g.tiles_n + g.tiles_n) % g.tiles_n;

    auto kstep = [&]() {
      const char* cur_a = smem + ca_slot * A_TILE_BYTES;
      const char* cur_b = smem + B_RING + cb_slot * B_TILE_BYTES;
      ca_slot = ca_slot + 1 == NA ? 0 : ca_slot + 1;
      cb_slot ^= 1;
      const bool rs_now = SPLITK && rowsum_on && rs_wait == 0;
#ifdef DEVIT_GEMM_NOCOMPUTE   // diagnostic build: the fill pipeline alone
      if (g.K < 0)
#endif
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        bf16x8 af[MI], bfr[NI];
#pragma unroll
        for (int j = 0; j < NI; ++j) bfr[j] = read_frag<B_KM, BN, PAIRED>(cur_b, wn * WN, j, kk, lane);
#pragma unroll
        for (int i = 0; i < MI; ++i) af[i] = read_frag<A_KM, BM, false>(cur_a, wm * WM, i, kk, lane);
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
          for (int j = 0; j < NI; ++j)
            acc[i][j] = DIRECT ? mfma16t<F16>(bfr[j], af[i], acc[i][j]) : mfma16t<F16>(af[i], bfr[j], acc[i][j]);
        if constexpr (SPLITK) {
          if (rs_now) {
#pragma unroll
            for (int i = 0; i < MI; ++i) rsum[i] = sum8_bf16(af[i], rsum[i]);
          }
        }
      }
      if constexpr (SPLITK) rs_wait = rs_wait == 0 ? g.tiles_n - 1 : rs_wait - 1;
    };
    const devit_epilogue& ep = g.ep;
    const int nw = ct.n0 + wn * WN;
    for (int t = 0; t < ct.nk - 1; ++t) {
      if (t > 0 || !primed) advance();
      kstep();
    }
    // last K-step of the tile: the epilogue's column data (bias, column scale) is fetched under its MFMAs
    if (ct.nk > 1 || !primed) advance();
    int noff[4];
    f32x4 bias[4], cs[4];
    if constexpr (DIRECT) load_cols<KIND>(ep, lane, nw, noff, bias, cs);
    kstep();
    if constexpr (DIRECT) settle_cols<KIND>(bias, cs);
    // The next tile's first stage is made readable BEFORE this tile's epilogue: a wait placed after the epilogue
    // would also wait for its stores (vmcnt retires in order), which a finishing workgroup never has to do.
    primed = DIRECT && tile + stride < last;
    if (primed) advance();

    const size_t ob = (size_t)ct.bz * ep.out_batch_stride;
    const int m_lim = ep.m_valid > 0 ? ep.m_valid : g.M;
    if constexpr (DIRECT) {
      // FULL: no row of the tile is padding -> straight-line code without per-row predicates (the predicated form makes
      // hipcc wait vmcnt(0) in front of every chunk: it cannot count stores across the skipped branches)
      if (ct.m0 + BM <= m_lim) epilogue_direct<KIND, MI, true, F16>(ep, acc, noff, bias, cs, lane, ct.m0 + wm * WM, m_lim, ob);
      else epilogue_direct<KIND, MI, false, F16>(ep, acc, noff, bias, cs, lane, ct.m0 + wm * WM, m_lim, ob);
    } else {
      // split-K partial sums: accumulators -> this wave's private 64x64 f32 LDS tile -> one atomic per element, 64
      // consecutive floats per instruction; one pass per 64 rows of the wave tile.  The ring is empty here
      // (the stream stops at tile ends for this kind).
      __syncthreads();  // all fragment reads done before the ring is reused as the staging area
      float* cw = (float*)smem + wave * 4096;
      float* out = (float*)ep.out + ob;
      // DET_F32: ep.out / ep.aux are the workspace; slab zz = batch * split_k + slice holds this tile's [M][N] partial, dense (ldc == N)
      const int zz = KIND == devit_gemm::DEVIT_EPI_DET_F32 ? fdiv(tile, g.d_per_z) : 0;
      if constexpr (KIND == devit_gemm::DEVIT_EPI_DET_F32) out = (float*)ep.out + (size_t)zz * g.M * g.N;
      auto do_pass = [&](auto pass_c) {
        constexpr int pass = decltype(pass_c)::value;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r)
              cw[(i * 16 + (lane >> 4) * 4 + r) * 64 + j * 16 + (lane & 15)] = acc[pass * 4 + i][j][r];
        // (same wave wrote and reads: the compiler's lgkmcnt wait orders them; no barrier needed)
        const int mw = ct.m0 + wm * WM + pass * 64;
        for (int row = 0; row < 64; ++row) {
          const float v = cw[row * 64 + lane];
          if constexpr (KIND == devit_gemm::DEVIT_EPI_DET_F32) {
            if (mw + row < m_lim) out[(size_t)(mw + row) * ep.ldc + nw + lane] = v;
          } else
#if defined(DEVIT_GEMM_NOATOMIC)  // ablation build: the split-K epilogue without its atomics
          if (mw + row < m_lim && v == 1.2345e30f) out[(size_t)(mw + row) * ep.ldc + nw + lane] = v;
#else
          if (mw + row < m_lim) unsafeAtomicAdd(out + (size_t)(mw + row) * ep.ldc + nw + lane, v);
#endif
        }
      };
      do_pass(std::integral_constant<int, 0>());
      if constexpr (MI > 4) do_pass(std::integral_constant<int, 1>());
      if (rowsum_on) {
        // lane l holds the partial sum of row (l & 15) over k = 8 (l >> 4) + 0..7 of every K-step: fold the four k groups
        float* rs_out = (float*)ep.aux;
#pragma unroll
        for (int i = 0; i < MI; ++i) {
          float v = rsum[i];
          v += __shfl_xor(v, 16, 64);
          v += __shfl_xor(v, 32, 64);
          const int row = ct.m0 + wm * WM + i * 16 + lane;
          if constexpr (KIND == devit_gemm::DEVIT_EPI_DET_F32) {   // partial (slice, n-tile): its own [M] row of the workspace behind the slabs
            if (lane < 16 && row < m_lim) rs_out[(size_t)(zz * g.tiles_n + ct.n0 / BN) * g.M + row] = v;
          } else
          if (lane < 16 && row < m_lim) unsafeAtomicAdd(rs_out + row, v);
        }
      }
      if (pb.tile < last) {          // restart the stream on the next tile
        __syncthreads();             // every wave's staging reads done before the DMA overwrites them
        pb.ref = decode_tile<BM, BN, A_KM, B_KM>(g, pb.tile);
        pb.t = 0;
        pb.open = true;
        pa = pb;
        a_slot = ca_slot;
        b_slot = cb_slot;
        issue_a();
        produce();
      }
    }
  }
}

// The (layout, epilogue) pairs the DeViT path uses on BM x BN tiles; anything else is DEVIT_ERR_ARG.
template <int BM, int BN, int WAVES_M, int WAVES_N, bool A_KM, bool B_KM, int KIND, bool F16 = false>
int launch_one(const GemmArgs& g, unsigned grid, hipStream_t s) {
  constexpr int ring = (3 * BM + 2 * BN) * 128, stagebytes = WAVES_M * WAVES_N * 16384;
  constexpr int lds = ((KIND == DEVIT_EPI_ATOMIC_F32 || KIND == devit_gemm::DEVIT_EPI_DET_F32) && stagebytes > ring) ? stagebytes : ring;
  return devit_gemm::launch_kernel<gemm_kernel<BM, BN, WAVES_M, WAVES_N, 2, A_KM, B_KM, KIND, F16>, lds>(grid, WAVES_M * WAVES_N * 64, s, g);
}
// forward layouts: bf16 or (ep.dtype16: the frozen teacher) f16 operands
template <int BM, int BN, int WAVES_M, int WAVES_N, int KIND>
int launch_fwd(const GemmArgs& g, unsigned grid, hipStream_t s) {
  return g.ep.dtype16 ? launch_one<BM, BN, WAVES_M, WAVES_N, false, false, KIND, true>(g, grid, s)
                      : launch_one<BM, BN, WAVES_M, WAVES_N, false, false, KIND, false>(g, grid, s);
}
template <int BM, int BN, int WAVES_M, int WAVES_N>
int launch_gemm_tile(const devit_gemm::GemmParams& p, int variant, unsigned grid, hipStream_t s) {
  const GemmArgs g{p};
  switch (variant * 16 + g.ep.kind) {
    case 0 * 16 + DEVIT_EPI_STORE_BF16: return launch_fwd<BM, BN, WAVES_M, WAVES_N, DEVIT_EPI_STORE_BF16>(g, grid, s);
    case 0 * 16 + DEVIT_EPI_STORE_F32: return launch_fwd<BM, BN, WAVES_M, WAVES_N, DEVIT_EPI_STORE_F32>(g, grid, s);
    case 0 * 16 + DEVIT_EPI_GELU_BF16: return launch_fwd<BM, BN, WAVES_M, WAVES_N, DEVIT_EPI_GELU_BF16>(g, grid, s);
    case 0 * 16 + DEVIT_EPI_RESIDUAL_F32: return launch_fwd<BM, BN, WAVES_M, WAVES_N, DEVIT_EPI_RESIDUAL_F32>(g, grid, s);
    case 0 * 16 + DEVIT_EPI_PATCH_F32: return launch_fwd<BM, BN, WAVES_M, WAVES_N, DEVIT_EPI_PATCH_F32>(g, grid, s);
    case 1 * 16 + DEVIT_EPI_STORE_BF16: return launch_one<BM, BN, WAVES_M, WAVES_N, false, true, DEVIT_EPI_STORE_BF16>(g, grid, s);
    case 1 * 16 + DEVIT_EPI_STORE_F32: return launch_one<BM, BN, WAVES_M, WAVES_N, false, true, DEVIT_EPI_STORE_F32>(g, grid, s);
    case 1 * 16 + DEVIT_EPI_DGELU_BF16: return launch_one<BM, BN, WAVES_M, WAVES_N, false, true, DEVIT_EPI_DGELU_BF16>(g, grid, s);
    case 3 * 16 + devit_gemm::DEVIT_EPI_DET_F32:
    case 3 * 16 + DEVIT_EPI_ATOMIC_F32:   // k-major x k-major never takes the 256x256 tile (gemm.hip's tile choice excludes it): not instantiated
    case 3 * 16 + DEVIT_EPI_STORE_F32:    // there (the 256x256 atomic kernel needed 257 registers: 1 spill)
      if constexpr (BM == 128) {
        if (g.ep.kind == DEVIT_EPI_ATOMIC_F32) return launch_one<BM, BN, WAVES_M, WAVES_N, true, true, DEVIT_EPI_ATOMIC_F32>(g, grid, s);
        if (g.ep.kind == devit_gemm::DEVIT_EPI_DET_F32) return launch_one<BM, BN, WAVES_M, WAVES_N, true, true, devit_gemm::DEVIT_EPI_DET_F32>(g, grid, s);
        return launch_one<BM, BN, WAVES_M, WAVES_N, true, true, DEVIT_EPI_STORE_F32>(g, grid, s);
      } else {
        devit_set_error("devit_gemm_bf16: k-major x k-major operands run on 128x128 tiles only");
        return DEVIT_ERR_ARG;
      }
    default:
      DEVIT_CHECK(false, DEVIT_ERR_ARG, "devit_gemm_bf16: layout %d with epilogue %d is not instantiated", variant, g.ep.kind);
  }
  return DEVIT_OK;
}

}  // namespace
