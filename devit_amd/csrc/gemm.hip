// Host side of the bf16 MFMA GEMM family: argument checks, the tile and kernel selection rules with the measurements behind them, and the C entry
// points devit_gemm_bf16, devit_gemm_route, devit_gemm_full_row_selected, devit_dgrad_layernorm_bwd(_fused), devit_set / get_reserved_cus.  The kernels and their
// launchers live in gemm_tile128.hip / gemm_tile256.hip (gemm_tile.h), gemm4.hip and gemmfr.hip; devit_wgrad_grouped in wgradfr.hip.
#include <stdlib.h>

#include "det.h"
#include "gemm_host.h"
#include "ln_rows.h"

using namespace devit_gemm;

namespace {
// CUs the persistent grids leave free (devit_set_reserved_cus): -1 = not set yet, take DEVIT_RESERVE_CUS from the environment
int g_reserved_cus = -1;
}  // namespace

int devit_gemm::reserved_cus() {
  if (g_reserved_cus < 0) {
    const char* e = getenv("DEVIT_RESERVE_CUS");
    int n = e ? atoi(e) : 0;
    g_reserved_cus = (n >= 0 && n <= 128) ? n / 8 * 8 : 0;
  }
  return g_reserved_cus;
}

int devit_gemm::cu_count() {
  static int cus = 0;
  if (cus == 0) {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n >= 8) cus = n;
  }
  return cus;
}
// workgroups of a persistent grid with `occ` of them per CU: a multiple of 8 (every XCD gets the same number), the reserved CUs left free
long long devit_gemm::persistent_grid(int cus, int occ) {
  const int avail = cus - reserved_cus() >= 8 ? cus - reserved_cus() : 8;
  return ((long long)avail * occ) / 8 * 8;
}
int devit_gemm::gemm_force() {    // DEVIT_GEMM_FORCE (tools/gpu_tiles.sh): 1 = 128x128 tiles for everything, 3 = 256x256 wherever built
  static const int exact = getenv("DEVIT_GEMM_FORCE") ? atoi(getenv("DEVIT_GEMM_FORCE")) : 0;
  return exact;
}

namespace {
// the LayerNorm backward fused into a launch (devit_dgrad_layernorm_bwd): the kernel's arguments and those of the column-sum pass behind it
struct FusedLnBwd {
  LnBwdArgs ln;
  float *dgamma, *dbeta, *dx_bf16_colsum;
  int accumulate;
};
int gemm_launch(const devit_operand* Aop, const devit_operand* Bop, int M, int N, int K, int batch, int split_k, const devit_epilogue* ep,
                const FusedLnBwd* ln, void* stream);
}  // namespace

// The full-row 256x384 kernel (gemmfr_kernel, gemmfr.hip): N == 384 exactly (one n-tile: its B stream is cyclic over the tiles), whole 256-row tiles and
// enough of them to give most CUs one (the token-row GEMMs of the lean last block stay on 128x128 tiles), K >= 3 stages.  In-step times,
// profiles/r05_*: the dgrads of qkv / proj / fc1 and fc2's forward; NOT proj's forward (6 K-steps in front of a 57 k-cycle residual epilogue on
// 198 of 256 CUs: slower than two 128x128 workgroups per CU), which therefore never passes a k-major weight.  DEVIT_GEMMFR=0 / 1 forces it
// off / on wherever it is built (read per call: tests switch it).
extern "C" int devit_gemm_full_row_selected(int M, int N, int K, int kind) {
  if (!(M > 0 && M % 256 == 0 && N == 384 && K % BK == 0 && K / BK >= 3 && (kind == DEVIT_EPI_RESIDUAL_F32 || kind == DEVIT_EPI_STORE_BF16)))
    return 0;
  const char* e = getenv("DEVIT_GEMMFR");
  return (e && *e) ? atoi(e) != 0 : M / 256 >= 64;    // (a minimum K of 1024 instead of 192 measured the same on the compacted student and 0.5 % less on the dense one)
}

extern "C" int devit_set_reserved_cus(int n) {
  DEVIT_CHECK(n >= 0 && n <= 128 && n % 8 == 0, DEVIT_ERR_ARG,
              "devit_set_reserved_cus: %d is not a multiple of 8 in [0, 128] (one share per XCD)", n);
  g_reserved_cus = n;
  return DEVIT_OK;
}

extern "C" int devit_get_reserved_cus(void) { return reserved_cus(); }

extern "C" int devit_gemm_bf16(const devit_operand* Aop, const devit_operand* Bop, int M, int N, int K, int batch,
                               int split_k, const devit_epilogue* ep, void* stream) {
  return gemm_launch(Aop, Bop, M, N, K, batch, split_k, ep, nullptr, stream);
}

namespace {
// What a launch runs on: the tile (cfg 1 = 128x128, 3 = 256x256, 4 = the full-row 256x384 kernel) and whether the four-wave kernel takes a 256x256
// launch.  as_enum() is what devit_gemm_route reports.
struct Route {
  int cfg, variant;
  bool use4;
  int as_enum() const { return cfg == 4 ? DEVIT_ROUTE_FULL_ROW : use4 ? DEVIT_ROUTE_GEMM4 : cfg == 3 ? DEVIT_ROUTE_TILE256 : DEVIT_ROUTE_TILE128; }
};

// Deterministic mode (det.h): an ATOMIC_F32 launch some of whose addresses receive more than one partial sum -- K slices onto the tile, (slice, n-tile)
// pairs onto the fused row sums -- runs the DET_F32 instantiation into the workspace, [batch][split_k] dense M x N slabs and behind them
// [split_k][tiles_n] rows of M sums, and fold launches add them to the destinations in index order.  Slice count and K ranges are the default's.
bool det_split(int N, int split_k, const devit_epilogue* ep) {
  return ep->kind == DEVIT_EPI_ATOMIC_F32 && (split_k > 1 || (ep->aux && N / 128 > 1)) && devit_det::on();
}
size_t det_slab_floats(int M, int N, int batch, int split_k) { return (size_t)batch * split_k * M * N; }
size_t det_bytes(int M, int N, int batch, int split_k, const devit_epilogue* ep) {
  return (det_slab_floats(M, N, batch, split_k) + (ep->aux ? (size_t)split_k * (N / 128) * M : 0)) * sizeof(float);
}

// The argument checks of devit_gemm_bf16 and THE selection rule of the family, in one place: gemm_launch launches what this says, devit_gemm_route
// reports it.  Host arithmetic and the environment only: no pointer is dereferenced but the three descriptors, nothing is launched, no device is asked.
int gemm_route(const devit_operand* Aop, const devit_operand* Bop, int M, int N, int K, int batch, int split_k, const devit_epilogue* ep, Route& r) {
  DEVIT_CHECK(Aop && Bop && Aop->ptr && Bop->ptr && ep && ep->out, DEVIT_ERR_ARG, "devit_gemm_bf16: null pointer");
  const void* A = Aop->ptr;
  const void* B = Bop->ptr;
  const int lda = Aop->ld, ldb = Bop->ld, a_kmajor = Aop->kmajor, b_kmajor = Bop->kmajor;
  DEVIT_CHECK(M > 0 && N > 0 && K > 0 && M % 128 == 0 && N % 128 == 0 && K % BK == 0 && batch >= 1, DEVIT_ERR_SHAPE,
              "devit_gemm_bf16: M=%d N=%d K=%d must be multiples of %d/%d/%d", M, N, K, 128, 128, BK);
  DEVIT_CHECK(lda % 8 == 0 && ldb % 8 == 0 && aligned16(A) && aligned16(B) && aligned16(ep->out) &&
                  ep->ldc % 8 == 0 && Aop->batch_stride % 8 == 0 && Bop->batch_stride % 8 == 0 &&
                  ep->out_batch_stride % 8 == 0,
              DEVIT_ERR_ARG, "devit_gemm_bf16: pointers / strides must be 16-byte aligned");
  DEVIT_CHECK(ep->kind >= DEVIT_EPI_STORE_BF16 && ep->kind <= DEVIT_EPI_STORE_F32, DEVIT_ERR_ARG,
              "devit_gemm_bf16: bad epilogue kind %d", ep->kind);
  DEVIT_CHECK(split_k >= 1 && (split_k == 1 || ep->kind == DEVIT_EPI_ATOMIC_F32) && split_k <= K / BK,
              DEVIT_ERR_ARG, "devit_gemm_bf16: split_k=%d only with ATOMIC_F32 and <= K/64", split_k);
  DEVIT_CHECK((a_kmajor ? lda >= M : lda >= K) && (b_kmajor ? ldb >= N : ldb >= K), DEVIT_ERR_ARG,
              "devit_gemm_bf16: leading dimension too small");
  DEVIT_CHECK((a_kmajor || Aop->row_group == 0) && (b_kmajor || Bop->row_group == 0), DEVIT_ERR_ARG,
              "devit_gemm_bf16: row_group/skip only for k-major operands");
  if (ep->kind == DEVIT_EPI_RESIDUAL_F32)
    DEVIT_CHECK(ep->res && (!ep->rowscale || ep->rows_per_scale > 0), DEVIT_ERR_ARG, "RESIDUAL: res / rows_per_scale");
  if (ep->kind == DEVIT_EPI_PATCH_F32)
    DEVIT_CHECK(ep->pos && ep->patch_tokens > 0 && (ep->m_valid > 0 ? ep->m_valid : M) % ep->patch_tokens == 0 && batch == 1,
                DEVIT_ERR_ARG,
                "PATCH: pos / tokens");
  if (ep->kind == DEVIT_EPI_DGELU_BF16)
    DEVIT_CHECK(ep->aux_in != nullptr && ep->bias == nullptr, DEVIT_ERR_ARG, "DGELU: needs aux_in, takes no bias (it is a dgrad)");
  if (ep->kind == DEVIT_EPI_ATOMIC_F32 && ep->aux)
    DEVIT_CHECK(batch == 1, DEVIT_ERR_ARG, "ATOMIC: the fused row sums of A (aux) need batch == 1");
  DEVIT_CHECK(ep->exact_gelu == 0, DEVIT_ERR_ARG, "devit_gemm_bf16: exact_gelu=1 (erff) is not built; the fused GELU is the "
              "fitted x * sigmoid(x * P(x^2)) form, |error| <= 2.6e-5 (devit_common.h); precision=\"f32\" uses erff");

  const bool f16 = ep->dtype16 != 0;
  DEVIT_CHECK(ep->dtype16 == 0 || ep->dtype16 == 1, DEVIT_ERR_ARG, "devit_gemm_bf16: dtype16 must be 0 (bf16) or 1 (f16)");
  DEVIT_CHECK(!f16 || (!a_kmajor && !b_kmajor && ep->kind != DEVIT_EPI_DGELU_BF16 && ep->kind != DEVIT_EPI_ATOMIC_F32),
              DEVIT_ERR_ARG, "devit_gemm_bf16: f16 operands are built for the forward layouts / epilogues only");
  // tile choice: 128x128 (4 waves, two workgroups per CU) or 256x256 (8 waves of 128x64, ping-pong schedule, one per CU)
  const int variant = (a_kmajor ? 2 : 0) + (b_kmajor ? 1 : 0);
  // Measured on the step's shapes (tools/gemm_tiles.py + tools/gpu_tiles.sh, M = 50688, TFLOP/s 256x256 vs 128x128):
  // the ping-pong 256x256 tile wins the long-K and plain-store shapes (teacher qkv 915-950 vs 838, fc2 K 3072 786 vs
  // 778) and the VALU-heavy GELU / dGELU epilogues at any K (student fc1 484 vs 452, teacher fc1 842 vs 817, fc2
  // dgrad 499 vs 481: one wave of each SIMD pair keeps the MFMA pipe while the other is in its epilogue only with two
  // workgroups per CU, but the fused GELU now costs less than the tile's extra fill traffic); the fp32 residual
  // epilogue at K <= 768 stays on 128x128 (teacher proj 458 vs 442), as does everything whose N is not a multiple
  // of 256 and the split-K wgrads.  (A 256x128 tile with a 3-deep ring and a 128x128 tile with a 3-deep ring at one
  // workgroup per CU were built and lost on every shape, warm and cold; they are gone.)
  const bool f16_in = ep->dtype16 != 0;       // (f16 operands run the eight-wave kernels only)
  const bool light_epi = ep->kind == DEVIT_EPI_STORE_BF16 || ep->kind == DEVIT_EPI_STORE_F32;
  const bool gelu_epi = ep->kind == DEVIT_EPI_GELU_BF16 || ep->kind == DEVIT_EPI_DGELU_BF16;
  int cfg = 1;
  // N = 256 k + 128 (student qkv: 1152) runs the 256-wide tile with a half-empty last n-tile: its B rows past N are
  // filled from row N-1 and the waves that own them skip the epilogue (variant 0, bf16 / f32 store only)
  // (also the GELU / dGELU epilogues: hidden 1152 = the compacted student's MLP width at shrink_ratio 0.3)
  const bool ragged_ok = ((variant == 0 && (light_epi || ep->kind == DEVIT_EPI_GELU_BF16)) ||
                          (variant == 1 && ep->kind == DEVIT_EPI_DGELU_BF16)) && N % 256 == 128 && N >= 1024;
  // plain-store launches take the 256x256 tile from this K on (round 4: student qkv, N 1152 K 384: 86 -> 70 us cold, 75 -> 70 in the step)
  constexpr int RAGGED_MIN_K = 384;
  // (the patch-embedding launch of a 768-wide model: 124 -> 108 us in the step on the larger tile; at N = 384 the 128x128 tile stays)
  const bool patch_wide = ep->kind == DEVIT_EPI_PATCH_F32 && K >= 768 && N % 256 == 0;
  // (the fp32 residual epilogue at K = 768, teacher proj: 125.9 us on 128x128 tiles, 120.3 on the four-wave 256x256 kernel, in the step)
  const bool resid_wide = ep->kind == DEVIT_EPI_RESIDUAL_F32 && K >= 768 && N % 256 == 0 && variant == 0 && !f16_in;
  if (M % 256 == 0 && (N % 256 == 0 || ragged_ok) && (K >= 1536 || (K >= RAGGED_MIN_K && light_epi) || gelu_epi || patch_wide || resid_wide) && variant != 3) cfg = 3;
  // too few 256x256 tiles to give every CU one (the token-row GEMMs of the lean last block, M = 512): 128x128 tiles
  // quarter the time of the longest workgroup; same accumulation order per output element either way
  if (cfg == 3 && (long long)(M / 256) * ((N + 255) / 256) * batch < 64) cfg = 1;
  const int exact = gemm_force();
  if (exact == 1 || (exact == 3 && M % 256 == 0 && (N % 256 == 0 || ragged_ok) && variant != 3)) cfg = exact;
  // the full-row 256x384 kernel: the student's N = 384 launches (round 5; per-shape times inside the step: profiles/r05_*).  DEVIT_GEMMFR=0 / 1
  // forces it off / on for everything it is built for (read per call: tests switch it).
  // (the kernel addresses B densely: a row-remapped k-major B stays on the 128x128 kernel, which honours row_group / row_skip -- except with the fp32
  // residual epilogue, which exists for a k-major B on this kernel only: refused below; DEVIT_GEMM_FORCE=1 means 128x128 tiles for everything)
  const bool b_dense = Bop->row_group == 0 && Bop->row_skip == 0;
  const bool use_fr = !f16 && split_k == 1 && batch == 1 && variant == 1 && b_dense && !(exact == 1 && ep->kind != DEVIT_EPI_RESIDUAL_F32) &&
                      devit_gemm_full_row_selected(M, N, K, ep->kind);
  DEVIT_CHECK(use_fr || !(variant == 1 && ep->kind == DEVIT_EPI_RESIDUAL_F32), DEVIT_ERR_ARG,
              "devit_gemm_bf16: the fp32 residual epilogue with a k-major weight runs on the full-row kernel only (N == 384, "
              "M %% 256 == 0, >= 64 row tiles, K >= 192, DEVIT_GEMMFR != 0, no row_group / row_skip on B): M=%d N=%d K=%d row_group=%d", M, N, K,
              Bop->row_group);
  if (use_fr) cfg = 4;
  // the four-wave kernel takes the 256x256 launches it is built for: row-major x row-major, whole 256-wide n-tiles, bf16
  // Which 256x256 launches take it (round 4, per-shape times inside the serialized step, tools/step_gemm_table.py): the two kernels
  // run their K loops at the same fill-bound rate (profiles/r04_a_gemm_four_wave.txt); the four-wave one is 2.5-3.4 % faster where the
  // epilogue is a plain bf16 store or the fp32 residual at K >= 768 (teacher qkv 172.6 -> 168.3 us, fc2 266 -> 257), and 5-10 % SLOWER
  // with the GELU epilogue (one wave per SIMD issues its vector instructions at half the rate two waves share) and on the batched
  // Gram launches.  DEVIT_GEMM4=0 / 1 forces it off / on for everything it is built for (read per call: tests switch it).
  const char* gemm4_env = getenv("DEVIT_GEMM4");
  const bool gemm4_ok = cfg == 3 && variant == 0 && !f16 && N % 256 == 0 && K / BK >= 3 && split_k == 1 &&
                        ep->kind != DEVIT_EPI_DGELU_BF16 && ep->kind != DEVIT_EPI_ATOMIC_F32;
  const bool gemm4_pays = (ep->kind == DEVIT_EPI_STORE_BF16 || ep->kind == DEVIT_EPI_RESIDUAL_F32) && K >= 768 && batch == 1;
  const bool use4 = gemm4_ok && (gemm4_env ? atoi(gemm4_env) != 0 : gemm4_pays);
  r.cfg = cfg;
  r.variant = variant;
  r.use4 = use4;
  const int bm = cfg == 1 ? 128 : 256, bn = cfg == 4 ? 384 : bm;
  DEVIT_CHECK((long long)(M / bm) * ((N + bn - 1) / bn) * split_k * batch < (1ll << 31), DEVIT_ERR_SHAPE, "devit_gemm_bf16: too many tiles");
  if (ep->kind == DEVIT_EPI_ATOMIC_F32 && batch > 1 && devit_det::on()) {
    // batches whose outputs overlap (out_batch_stride smaller than one output) are further partial sums per address that no slice index orders
    const long long m_lim = ep->m_valid > 0 ? ep->m_valid : M;
    DEVIT_CHECK(ep->out_batch_stride >= (m_lim - 1) * (long long)ep->ldc + N, DEVIT_ERR_ARG,
                "devit_gemm_bf16: deterministic mode refuses ATOMIC_F32 with batch=%d whose outputs overlap (out_batch_stride=%lld): the batches would "
                "add into one address in arrival order", batch, ep->out_batch_stride);
  }
  if (det_split(N, split_k, ep)) return devit_det::workspace("devit_gemm_bf16", det_bytes(M, N, batch, split_k, ep), nullptr);
  return DEVIT_OK;
}

// devit_gemm_bf16; with `ln`, the launch whose bf16 output feeds the LayerNorm backward `ln` in the same kernel (devit_dgrad_layernorm_bwd: the
// caller has checked devit_dgrad_layernorm_bwd_fused, anything else is an error here, never a silent other path)
int gemm_launch(const devit_operand* Aop, const devit_operand* Bop, int M, int N, int K, int batch, int split_k, const devit_epilogue* ep,
                const FusedLnBwd* ln, void* stream) {
  Route route;
  const int rc_route = gemm_route(Aop, Bop, M, N, K, batch, split_k, ep, route);
  if (rc_route != DEVIT_OK) return rc_route;
  const int cfg = route.cfg, variant = route.variant, a_kmajor = Aop->kmajor, b_kmajor = Bop->kmajor;
  const bool use4 = route.use4;
  GemmParams g;
  g.A = (const __bf16*)Aop->ptr; g.B = (const __bf16*)Bop->ptr;
  g.lda = Aop->ld; g.ldb = Bop->ld;
  g.a_group = Aop->row_group; g.a_skip = Aop->row_skip; g.b_group = Bop->row_group; g.b_skip = Bop->row_skip;
  g.a_bs = Aop->batch_stride; g.b_bs = Bop->batch_stride;
  g.M = M; g.N = N; g.K = K;
  g.tiles_m = 0; g.tiles_n = 0; g.split_k = split_k;
  g.ep = *ep;
  const bool det = det_split(N, split_k, ep);
  if (det) {
    float* ws = nullptr;
    const int rc = devit_det::workspace("devit_gemm_bf16", det_bytes(M, N, batch, split_k, ep), &ws);
    if (rc != DEVIT_OK) return rc;
    g.ep.kind = DEVIT_EPI_DET_F32;
    g.ep.out = ws;
    g.ep.ldc = N;
    g.ep.out_batch_stride = 0;
    if (ep->aux) g.ep.aux = ws + det_slab_floats(M, N, batch, split_k);
  }
  const int bm = cfg == 1 ? 128 : 256, bn = cfg == 4 ? 384 : bm;
  g.tiles_m = M / bm;
  g.tiles_n = (N + bn - 1) / bn;
  {
    // Tile order inside an XCD: n-tile fastest inside chunks of gn n-tiles, so that the W workgroups an XCD runs at
    // the same time cover about W / gn m-tiles x gn n-tiles and share their operand panels through the XCD's L2 while
    // they walk K together.  Fill bytes per K-step are ~ (W / gn) BM + gn BN: smallest near gn = sqrt(W BM / BN)
    // (8 for two 128x128 workgroups on each of the 32 CUs, 6 for one 256x256).  Measured with FETCH_SIZE on the
    // teacher fc2 GEMM (K = 3072, three 256-wide n-tiles): gn = 1 fetched the activation panel once per n-tile
    // (1137 MB per launch against 472 MB algorithmic).
    static const int gn_env = getenv("DEVIT_GEMM_GN") ? atoi(getenv("DEVIT_GEMM_GN")) : 0;
    const int per_xcd = (cfg == 1 ? 64 : 32);
    int target = 1;
    while ((target + 1) * (target + 1) * bn <= per_xcd * bm + (target + 1) * bn) ++target;   // ~ round(sqrt(W BM / BN))
    const int nchunks = (g.tiles_n + target - 1) / target;
    g.gn = gn_env > 0 ? gn_env : (g.tiles_n + nchunks - 1) / nchunks;
    if (g.gn > g.tiles_n) g.gn = g.tiles_n;
  }
  const long long tiles = (long long)g.tiles_m * g.tiles_n * split_k * batch;
  g.total_tiles = (int)tiles;
  g.d_per_z = make_fastdiv(g.tiles_m * g.tiles_n);
  g.d_chunk = make_fastdiv(g.gn * g.tiles_m);
  g.d_gn = make_fastdiv(g.gn);
  g.d_last = make_fastdiv(g.tiles_n % g.gn ? g.tiles_n % g.gn : g.gn);
  g.d_split = make_fastdiv(split_k);
  // persistent grid: as many workgroups as stay resident (LDS: two 128x128 rings or one 256-wide ring per CU), a
  // multiple of 8 so that every XCD gets the same number
  const int cus = cu_count();
  DEVIT_CHECK(cus >= 8, DEVIT_ERR_DEVICE, "devit_gemm_bf16: cannot query the CU count");
  static const int occ_env = getenv("DEVIT_GEMM_OCC") ? atoi(getenv("DEVIT_GEMM_OCC")) : 0;
  const int occ = cfg == 4 ? 1 : occ_env > 0 ? occ_env : (cfg == 1 ? 2 : 1);
  // A persistent grid holds every CU it starts on (the 256x256 workgroup owns the CU's whole LDS and register file) until
  // its last tile: a collective's kernels launched meanwhile (RCCL on the exchange stream) wait for a GEMM to END, and once
  // they hold CUs the next 256-workgroup grid runs a second, nearly empty round.  With `reserved` CUs left free the grid
  // is smaller and its tiles are dealt over the workgroups that do run (devit_set_reserved_cus; 0 at world size 1).
  long long nwg = persistent_grid(cus, occ);
  DEVIT_CHECK(!ln || (cfg == 4 && ep->kind == DEVIT_EPI_STORE_BF16 && tiles <= nwg), DEVIT_ERR_ARG,
              "the fused dgrad + LayerNorm-backward launch needs the full-row kernel and one tile per workgroup: M=%d K=%d", M, K);
  if (nwg > (tiles + 7) / 8 * 8) nwg = (tiles + 7) / 8 * 8;
  hipStream_t s = (hipStream_t)stream;
  auto info = [&] {
    devit_launch_info i = {ln ? "devit_dgrad_layernorm_bwd" : "devit_gemm_bf16"};
    i.a_kmajor = a_kmajor != 0; i.b_kmajor = b_kmajor != 0; i.kind = ep->kind;
    i.M = M; i.N = N; i.K = K; i.batch = batch; i.split_k = split_k;
    return i;
  };
  return devit_observed(stream, info, [&]() -> int {
    if (cfg == 4) {
      const int rc = launch_gemmfr(g, ln ? &ln->ln : nullptr, (unsigned)nwg, s);
      if (rc != DEVIT_OK || !ln) return rc;
      // (one partial per tile: <= CUs <= the rows / 8 (or 1024) parts the workspace is sized for)
      return devit_layernorm_bwd_finish(ln->ln.partial, g.tiles_m, N, ln->dgamma, ln->dbeta, ln->dx_bf16_colsum, ln->accumulate, stream);
    }
    if (use4) return launch_gemm4(g, (unsigned)nwg, s);
    if (!det) return cfg == 3 ? launch_gemm_tile256(g, variant, (unsigned)nwg, s) : launch_gemm_tile128(g, variant, (unsigned)nwg, s);
    int rc = launch_gemm_tile128(g, variant, (unsigned)nwg, s);
    const int m_lim = ep->m_valid > 0 ? ep->m_valid : M;
    if (rc == DEVIT_OK) rc = devit_det::fold((const float*)g.ep.out, split_k, (size_t)M * N, m_lim, N, (float*)ep->out, ep->ldc, batch, ep->out_batch_stride, s);
    if (rc == DEVIT_OK && ep->aux) rc = devit_det::fold((const float*)g.ep.aux, split_k * g.tiles_n, (size_t)M, 1, m_lim, (float*)ep->aux, 0, 1, 0, s);
    return rc;
  });
}
}  // namespace

// What devit_gemm_bf16 would run this call on (DEVIT_ROUTE_*), or the DEVIT_ERR_* of its argument checks: gemm_route itself, nothing launched
extern "C" int devit_gemm_route(const devit_operand* A, const devit_operand* B, int M, int N, int K, int batch, int split_k, const devit_epilogue* ep) {
  Route r;
  const int rc = gemm_route(A, B, M, N, K, batch, split_k, ep, r);
  return rc != DEVIT_OK ? rc : r.as_enum();
}

// Would devit_dgrad_layernorm_bwd take the fused launch?  The rule, in one place: the full-row kernel would run the product (N = D = 384, whole
// 256-row tiles and enough of them, DEVIT_GEMMFR / DEVIT_GEMM_FORCE not against it) AND every workgroup of its grid gets at most one tile -- with a
// next tile the operand ring holds that tile's prefetched stages and there is no LDS to stage rows in.  DEVIT_LNFUSE=0 (read per call: tests switch
// it) forces the two unfused launches.
extern "C" int devit_dgrad_layernorm_bwd_fused(int M_pad, int D, int K) {
  const char* e = getenv("DEVIT_LNFUSE");
  if (e && *e && atoi(e) == 0) return 0;
  if (D != 384 || gemm_force() == 1 || !devit_gemm_full_row_selected(M_pad, D, K, DEVIT_EPI_STORE_BF16)) return 0;
  const int cus = cu_count();
  return cus >= 8 && M_pad / 256 <= persistent_grid(cus, 1);
}

extern "C" int devit_dgrad_layernorm_bwd(const void* dy, const void* w, int M_pad, int K, void* dln, const float* x, int rows, int D,
                                         const float* mean, const float* rstd, const float* gamma, const float* dres, float* dx,
                                         void* dx_bf16, const float* rowscale, int rows_per_scale, float* dgamma, float* dbeta,
                                         float* dx_bf16_colsum, int accumulate, void* workspace, size_t workspace_bytes, void* stream) {
  DEVIT_CHECK(dy && w && dln && rows > 0 && rows <= M_pad, DEVIT_ERR_ARG, "devit_dgrad_layernorm_bwd: bad argument");
  devit_operand A = {dy, K, 0, 0, 0, 0}, Bo = {w, D, 1, 0, 0, 0};
  devit_epilogue ep = {};
  ep.kind = DEVIT_EPI_STORE_BF16;
  ep.out = dln;
  ep.ldc = D;
  ep.m_valid = rows;
  if (!devit_dgrad_layernorm_bwd_fused(M_pad, D, K)) {
    int rc = devit_gemm_bf16(&A, &Bo, M_pad, D, K, 1, 1, &ep, stream);
    if (rc != DEVIT_OK) return rc;
    return devit_layernorm_bwd(dln, 0, x, rows, D, 0, 0, mean, rstd, gamma, dres, dx, dx_bf16, rowscale, rows_per_scale, dgamma, dbeta,
                               dx_bf16_colsum, accumulate, workspace, workspace_bytes, stream);
  }
  // (devit_layernorm_bwd's argument checks)
  DEVIT_CHECK(x && mean && rstd && gamma && dx && dgamma && dbeta && workspace, DEVIT_ERR_ARG, "devit_dgrad_layernorm_bwd: null pointer");
  DEVIT_CHECK(workspace_bytes >= devit_layernorm_bwd_workspace(rows, D), DEVIT_ERR_ARG, "devit_dgrad_layernorm_bwd: workspace too small");
  DEVIT_CHECK(!rowscale || rows_per_scale > 0, DEVIT_ERR_ARG, "devit_dgrad_layernorm_bwd: rows_per_scale");
  DEVIT_CHECK(!dx_bf16_colsum || dx_bf16, DEVIT_ERR_ARG, "devit_dgrad_layernorm_bwd: dx_bf16_colsum needs dx_bf16");
  DEVIT_CHECK(aligned16(x) && aligned16(dx) && (!dres || aligned16(dres)) && (!dx_bf16 || aligned16(dx_bf16)), DEVIT_ERR_ARG,
              "devit_dgrad_layernorm_bwd: x / dres / dx / dx_bf16 must be 16-byte aligned");
  const FusedLnBwd ln{{nullptr, x, mean, rstd, gamma, dres, dx, (__bf16*)dx_bf16, rowscale, rows_per_scale, (float*)workspace, rows, D, 0, 0, 0},
                      dgamma, dbeta, dx_bf16_colsum, accumulate};
  return gemm_launch(&A, &Bo, M_pad, D, K, 1, 1, &ep, &ln, stream);
}
