// wgradfr_kernel and its C entry points.
#include "det.h"
#include "gemm_device.h"

using namespace devit_gemm;

namespace {

#include "gemmfr_kloop.inc"   // DEVIT_WGRADFR_KLOOP_*, gemmfr_read_acc

// ---------------------------------------------------------------------------------------------------------------------
// Weight gradients on the full-row tile (round 6): out (+)= A^T B over the token rows, BOTH operands k-major ([K][features], as the step holds
// dY and X), a table of up to WGRAD_MAX_JOBS jobs = the Linear layers of one block (or of several) in ONE launch, one 256 x 384 tile and one K slice per
// workgroup, all of them resident at once.  Why: the split-K 128x128 launches this replaces (four per block) asked the CU's fill path for
// 64 B per cycle of matrix pipe where it delivers ~24 and ran 14-56-step K loops in front of 64 KB of atomics each;
// this tile needs 26.7 B per cycle, reads the dY panel once, and a block's four products are 19 tiles x 13 slices = 247 workgroups with
// ~61-step K loops.  K loop: the generated asm statement DEVIT_WGRADFR_KLOOP (tools/gen_gemmfr.py, KMA variant: the ring protocol, phases and
// waits of gemmfr_kernel; A image [64 k][256], fragments by ds_read_b64_tr_b16 on both sides, PAIRED tile-row order on both sides, column
// sums of A by v_dot2c against packed ones).  Epilogue: the accumulators go through LDS 32 rows at a time and leave as fp32 atomics on whole
// 256-byte rows (128-byte columns for a transposed job).
constexpr int WGRAD_MAX_JOBS = 48;
struct WgJob {
  const __bf16* a;
  const __bf16* b;
  float* out;
  float* colsum;
  int lda, ldb, ldc, a_cols, transposed, tile0;    // tile0: index of the job's first tile in the table's tile list
};
struct WgArgs {
  WgJob job[WGRAD_MAX_JOBS];
  int njobs, tiles, split, nk_total, total;
  unsigned long long* dbg;       // stamped diagnostic build only (tools/wgradfr_stamps.py)
};

struct WgDetArgs : WgArgs {
  float* ws;      // deterministic mode: [split][tiles][256][384] partial tiles, then [split][tiles][256] partial column sums of A
};

#define WGRADFR_KERNEL wgradfr_kernel
#define WGRADFR_DET 0
#include "wgradfr_kernel.inc"
#undef WGRADFR_KERNEL
#undef WGRADFR_DET
#define WGRADFR_KERNEL wgradfr_det_kernel
#define WGRADFR_DET 1
#include "wgradfr_kernel.inc"
#undef WGRADFR_KERNEL
#undef WGRADFR_DET

// Deterministic mode, behind wgradfr_det_kernel: out (+)= the K slices' partial tiles folded in slice order (det.h), one thread per element;
// grid (tiles, 32): a workgroup takes 8 rows (= A columns) of its tile, a transposed job's element goes to out[col][row].  The y == 0 workgroups
// also fold the tile's partial column sums.
__global__ __launch_bounds__(256) void wgrad_fold_kernel(const WgDetArgs g) {
  constexpr int BM = 256, BN = 384;
  const int t = blockIdx.x;
  int ji = 0;
  for (int j = 1; j < g.njobs; ++j)
    if (t >= g.job[j].tile0) ji = j;
  const WgJob& jb = g.job[ji];
  const int m0 = (t - jb.tile0) * BM;
  const int valid = min(BM, jb.a_cols - m0);
  const size_t slab = (size_t)g.tiles * BM * BN;
  for (int i = threadIdx.x; i < 8 * BN; i += 256) {
    const int r = blockIdx.y * 8 + i / BN, c = i % BN;
    if (r >= valid) continue;
    const float* p = g.ws + ((size_t)t * BM + r) * BN + c;
    float f = p[0];
    for (int z = 1; z < g.split; ++z) f += p[(size_t)z * slab];
    float* o = jb.transposed ? jb.out + (size_t)c * jb.ldc + m0 + r : jb.out + (size_t)(m0 + r) * jb.ldc + c;
    *o = *o + f;
  }
  if (blockIdx.y == 0 && jb.colsum && (int)threadIdx.x < valid) {
    const float* p = g.ws + (size_t)g.total * (BM * BN) + (size_t)t * BM + threadIdx.x;
    float f = p[0];
    for (int z = 1; z < g.split; ++z) f += p[(size_t)z * g.tiles * BM];
    jb.colsum[m0 + threadIdx.x] += f;
  }
}

}  // namespace

#ifdef DEVIT_GEMMFR_STAMP
static unsigned long long* g_wgrad_dbg = nullptr;
extern "C" DEVIT_API void devit_wgrad_debug_buffer(void* p) { g_wgrad_dbg = (unsigned long long*)p; }   // [grid x 4 waves x 8] u64, diagnostic build only
#endif

extern "C" int devit_wgrad_grouped(const devit_wgrad_job* jobs, int njobs, int K, int split_k, void* stream) {
  DEVIT_CHECK(jobs && njobs >= 1 && njobs <= WGRAD_MAX_JOBS, DEVIT_ERR_ARG, "devit_wgrad_grouped: 1..%d jobs (host array)", WGRAD_MAX_JOBS);
  DEVIT_CHECK(K > 0 && K % BK == 0, DEVIT_ERR_SHAPE, "devit_wgrad_grouped: K=%d must be a multiple of %d", K, BK);
  WgArgs g;
  int tiles = 0;
  for (int j = 0; j < njobs; ++j) {
    const devit_wgrad_job& q = jobs[j];
    DEVIT_CHECK(q.a && q.b && q.out, DEVIT_ERR_ARG, "devit_wgrad_grouped: job %d: null pointer", j);
    DEVIT_CHECK(q.a_cols > 0 && q.a_cols % 128 == 0 && q.lda >= q.a_cols && q.ldb >= 384 && q.lda % 8 == 0 && q.ldb % 8 == 0, DEVIT_ERR_SHAPE,
                "devit_wgrad_grouped: job %d: a_cols=%d (a multiple of 128) lda=%d ldb=%d (>= 384 columns are read)", j, q.a_cols, q.lda, q.ldb);
    DEVIT_CHECK(aligned16(q.a) && aligned16(q.b) && ((uintptr_t)q.out & 3) == 0 && q.ldc >= (q.transposed ? q.a_cols : 384), DEVIT_ERR_ARG,
                "devit_wgrad_grouped: job %d: operands must be 16-byte aligned, ldc=%d too small", j, q.ldc);
    g.job[j] = WgJob{(const __bf16*)q.a, (const __bf16*)q.b, q.out, q.a_colsum, q.lda, q.ldb, q.ldc, q.a_cols, q.transposed, tiles};
    tiles += (q.a_cols + 255) / 256;
  }
  const int cus = cu_count();
  DEVIT_CHECK(cus >= 8, DEVIT_ERR_DEVICE, "devit_wgrad_grouped: cannot query the CU count");
  const int nk_total = K / BK;
  if (split_k <= 0) {
    // K slices by a two-term cost model (microseconds), both terms measured (profiles/r06_a_wgradfr_*.txt, r06_H_*): a workgroup walks a K-step in
    // ~2.1 us (the launch is bound by the LDS-DMA stream out of HBM), workgroups run one per CU in rounds of `avail`; every (tile, slice) leaves through
    // 384 KB of fp32 atomics, which the memory side retires at ~1.3 TB/s chip-wide whoever issues them (0.30 us each).  One block: 19 tiles -> 13 slices
    // (202 us modelled, 200-230 measured); eleven blocks: 209 tiles -> no split (1723 / 1720); a compacted student's 162 tiles -> 3 slices (two rounds
    // of a third of the K loop instead of one round on 162 of 256 CUs).
    const int avail = cus - reserved_cus() >= 8 ? cus - reserved_cus() : 8;
    int best = 1;
    double best_cost = 1e30;
    for (int sk = 1; sk <= 64 && nk_total / sk >= 3; ++sk) {
      const long long units = (long long)tiles * sk;
      const double rounds = (double)((units + avail - 1) / avail);
      const double cost = 2.1 * ((nk_total + sk - 1) / sk) * rounds + 0.30 * (double)units;
      if (cost < best_cost - 1e-9) {
        best_cost = cost;
        best = sk;
      }
    }
    split_k = best;
  }
  DEVIT_CHECK(split_k >= 1 && nk_total / split_k >= 3, DEVIT_ERR_SHAPE, "devit_wgrad_grouped: K=%d gives %d K-steps, fewer than 3 per slice at split_k=%d",
              K, nk_total, split_k);
  g.njobs = njobs; g.tiles = tiles; g.split = split_k; g.nk_total = nk_total; g.total = tiles * split_k;
#ifdef DEVIT_GEMMFR_STAMP
  g.dbg = g_wgrad_dbg;
#else
  g.dbg = nullptr;
#endif
  constexpr int lds = (256 + 384) * 128 * 2;
  auto info = [&] {
    devit_launch_info i = {"devit_wgrad_grouped"};
    i.a_kmajor = i.b_kmajor = 1; i.kind = DEVIT_EPI_ATOMIC_F32; i.K = K; i.split_k = split_k; i.njobs = njobs;
    for (int j = 0; j < njobs; ++j) i.a_cols += jobs[j].a_cols;
    i.flops = 2.0 * K * i.a_cols * 384;
    i.bytes = (double)K * (i.a_cols + 384 * njobs) * 2 + (double)i.a_cols * 384 * 4;
    return i;
  };
  // Deterministic mode: one slice adds ONE partial per address (fp32 addition onto the destination: order-free); more go through the workspace, with the
  // default's slice count and K ranges
  const bool det = split_k > 1 && devit_det::on();
  WgDetArgs gd;
  if (det) {
    static_cast<WgArgs&>(gd) = g;
    const int rc = devit_det::workspace("devit_wgrad_grouped", (size_t)g.total * (256 * 384 + 256) * sizeof(float), &gd.ws);
    if (rc != DEVIT_OK) return rc;
  }
  return devit_observed(stream, info, [&]() -> int {
    if (!det) return launch_kernel<wgradfr_kernel, lds>((unsigned)((g.total + 7) / 8 * 8), 256, (hipStream_t)stream, g);
    const int rc = launch_kernel<wgradfr_det_kernel, lds>((unsigned)((g.total + 7) / 8 * 8), 256, (hipStream_t)stream, gd);
    if (rc != DEVIT_OK) return rc;
    hipLaunchKernelGGL(wgrad_fold_kernel, dim3(g.tiles, 32), dim3(256), 0, (hipStream_t)stream, gd);
    DEVIT_LAUNCH_CHECK();
    return DEVIT_OK;
  });
}
