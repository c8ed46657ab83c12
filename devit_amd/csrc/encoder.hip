// Whole encoder blocks per host call (devit_encoder_fwd / devit_block_bwd, and devit_tail_fwd / devit_tail_bwd for the lean last block): the
// block's kernels are enqueued here, in C++, through the single-kernel entry points of the C ABI.  This is the ONE host sequence of the 16-bit
// block: the Python side (devit_amd/ops.py) holds no restatement of it, and what instruments need to see of it -- which GEMM, LayerNorm,
// attention and weight-gradient launches, on which stream -- those entry points report to the launch observer (devit_set_launch_observer).
// The block is written in two halves: the attention half (LN1, qkv, attention) and the branch half (proj + residual, LN2, fc1, fc2 + residual;
// branch_fwd / branch_bwd).  The lean last block has an attention half of its own -- K and V on all rows, Q and everything behind it on the
// token rows -- and runs the SAME branch half on its token rows.
// devit_block_bwd puts its four weight-gradient launches on a side stream of its own and joins it before it returns (round 4,
// see there).  Host code only.
#include <mutex>

#include "det.h"
#include "devit_common.h"

namespace {

inline int pad_rows(int m) { return (m + 255) / 256 * 256; }
inline size_t align256(size_t b) { return (b + 255) / 256 * 256; }

// split-K factor of a weight-gradient GEMM: one round of resident 128x128 workgroups (two per CU), see ops.split_k_for
inline int split_k_for(int out_rows, int out_cols, int ksteps) {
  const int tiles = (out_rows / 128) * (out_cols / 128);
  int s = 512 / (tiles > 0 ? tiles : 1);
  if (s > ksteps) s = ksteps;
  return s < 1 ? 1 : s;
}

struct Ctx {
  int M, Mp, B, N, D;
  float eps;
  void* stream;
};

// DEVIT_BLK_QKV_PAD: zeroed rows behind the padded qkv buffer.  The relation loss reads a 256-row Gram window per image, the last one from row
// (B - 1) N on: 256 - N rows behind the B N live ones -- 58 at N = 198, inside the 128 every N >= 128 gets; a short sequence (51 tokens of a
// 112-pixel model) gets its 256 - N.
inline int qkv_pad_rows(int N) { return N >= 128 ? 128 : 256 - N; }

int zero_pad(const Ctx& c, void* buf, int cols, size_t elem, int extra_rows = 0) {
  if (!buf) return DEVIT_OK;
  const int rows = c.Mp + extra_rows - c.M;
  if (rows <= 0) return DEVIT_OK;
  hipError_t e = hipMemsetAsync((char*)buf + (size_t)c.M * cols * elem, 0, (size_t)rows * cols * elem, (hipStream_t)c.stream);
  DEVIT_CHECK(e == hipSuccess, DEVIT_ERR_LAUNCH, "hipMemsetAsync: %s", hipGetErrorString(e));
  return DEVIT_OK;
}

devit_epilogue make_ep(int kind, void* out, int ldc, int m_valid, int dtype16 = 0) {
  devit_epilogue ep = {};
  ep.kind = kind;
  ep.out = out;
  ep.ldc = ldc;
  ep.m_valid = m_valid;
  ep.dtype16 = dtype16;
  return ep;
}

// out[M][Nout] = x[Mp][K] @ w[Nout][K]^T (+ epilogue)
int linear_fwd(const Ctx& c, const void* x, const void* w, int Nout, int K, devit_epilogue ep) {
  devit_operand A = {x, K, 0, 0, 0, 0}, Bo = {w, K, 0, 0, 0, 0};
  return devit_gemm_bf16(&A, &Bo, c.Mp, Nout, K, 1, 1, &ep, c.stream);
}
// out[M][K] = dy[Mp][Nw] @ w[Nw][K]   (w read k-major)
int linear_dgrad(const Ctx& c, const void* dy, const void* w, int Nw, int K, devit_epilogue ep) {
  devit_operand A = {dy, Nw, 0, 0, 0, 0}, Bo = {w, K, 1, 0, 0, 0};
  return devit_gemm_bf16(&A, &Bo, c.Mp, K, Nw, 1, 1, &ep, c.stream);
}
// w_grad[Nw][K] += dy[Mp][Nw]^T @ x[Mp][K]; b_grad[Nw] += column sums of dy (same launch)
// (ld_dy: dy's leading dimension where it is a column block of a wider matrix; 0 = Nw)
int linear_wgrad(const Ctx& c, const void* dy, const void* x, float* w_grad, float* b_grad, int Nw, int K, int ld_dy = 0) {
  devit_operand A = {dy, ld_dy ? ld_dy : Nw, 1, 0, 0, 0}, Bo = {x, K, 1, 0, 0, 0};
  devit_epilogue ep = make_ep(DEVIT_EPI_ATOMIC_F32, w_grad, K, 0);
  ep.aux = b_grad;
  return devit_gemm_bf16(&A, &Bo, Nw, K, c.Mp, 1, split_k_for(Nw, K, c.Mp / 64), &ep, c.stream);
}

// The block's weight gradients as jobs of ONE devit_wgrad_grouped launch (the full-row weight-gradient kernel, wgradfr.hip): possible when
// one side of every product is exactly 384 features wide (D == 384: the student) and the other a multiple of 128.
//   dW[Nw][K] += dy^T x:   K == 384 -> tiles over dy's features (column sums of dy = the bias gradient from the same launch);
//                          Nw == 384 -> the product transposed, tiles over x's features (no bias gradient: the caller has it from elsewhere)
bool wgrad_job(devit_wgrad_job* j, const void* dy, const void* x, float* w_grad, float* b_grad, int Nw, int K) {
  if (K == 384 && Nw % 128 == 0) {
    *j = devit_wgrad_job{dy, Nw, Nw, x, K, w_grad, K, 0, b_grad};
    return true;
  }
  if (Nw == 384 && K % 128 == 0 && b_grad == nullptr) {
    *j = devit_wgrad_job{x, K, K, dy, Nw, w_grad, K, 1, nullptr};
    return true;
  }
  return false;
}
// DEVIT_WGRADFR (read per call: tests switch it): 0 = four split-K launches on 128x128 tiles (rounds 1-5); else (default) the grouped launch
// (two launches per block -- the MLP pair behind the fc1 dgrad, the attention pair behind the qkv dgrad, for the Infinity Cache -- measured
// 4 % slower on the step than one: twice the atomics)
int wgrad_mode(const Ctx& c) {
  if (!(c.D == 384 && c.Mp / 64 >= 3)) return 0;
  const char* e = getenv("DEVIT_WGRADFR");
  return (e && *e) ? atoi(e) != 0 : 1;
}

#define TRY(x)                 \
  do {                         \
    int rc__ = (x);            \
    if (rc__ != DEVIT_OK) return rc__; \
  } while (0)

// devit_block_bwd's side stream for the weight-gradient launches: one per device, created at the first call that wants it (once, under
// std::call_once: two host threads making their first call together see one stream), owned by the library for the life of the process
// (declared at devit_block_bwd in include/devit_hip.h).  A device index past the table runs without one (= on the caller's stream).
struct WgradSide {
  hipStream_t stream;
  hipEvent_t ev[5];
  bool ok = false;
};
constexpr int MAX_DEVICES = 16;
int wgrad_side(WgradSide** out) {
  const char* env = getenv("DEVIT_WGRAD_STREAM");      // (read per call: tests switch it)
  // (deterministic mode keeps them on `stream` too: one stream orders every launch that uses the registered workspace, det.h)
  const bool on = !(env && atoi(env) == 0) && !devit_det::on();
  static WgradSide per_dev[MAX_DEVICES];
  static std::once_flag once[MAX_DEVICES];
  *out = nullptr;
  if (!on) return DEVIT_OK;
  int dev = 0;
  DEVIT_CHECK(hipGetDevice(&dev) == hipSuccess && dev >= 0, DEVIT_ERR_DEVICE, "devit_block_bwd: hipGetDevice");
  if (dev >= MAX_DEVICES) return DEVIT_OK;
  std::call_once(once[dev], [dev]() {
    WgradSide& s = per_dev[dev];
    if (hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking) != hipSuccess) return;
    for (auto& e : s.ev)
      if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return;
    s.ok = true;
  });
  DEVIT_CHECK(per_dev[dev].ok, DEVIT_ERR_DEVICE, "devit_block_bwd: cannot create the weight-gradient stream / its events");
  *out = &per_dev[dev];
  return DEVIT_OK;
}

int check_dims(int B, int N, int D, int Da, int Hd) {
  DEVIT_CHECK(B > 0 && N > 0 && N <= 208 && D > 0 && D % 128 == 0 && Da > 0 && Da % 128 == 0 && Hd > 0 && Hd % 128 == 0,
              DEVIT_ERR_SHAPE, "block: B=%d N=%d D=%d attn_width=%d hidden=%d not supported", B, N, D, Da, Hd);
  return DEVIT_OK;
}

// The branch half of the forward, from the proj GEMM on: x1 = x + dp1 * proj(attn_o); x2 = x1 + dp2 * fc2(gate * gelu(fc1(ln2(x1)))), on the c.M
// rows of `x` and of a's buffers, c.N rows per DropPath scale.  block_fwd runs it on all rows (x = a.x), tail_fwd on the token rows (x = the
// gathered ones).  The caller has checked the buffers and the dropout arguments; d as for block_fwd.
int branch_fwd(const Ctx& c, const devit_block_weights& w, const float* x, const devit_block_acts& a, const devit_block_dropout* d) {
  const int D = c.D, Da = w.attn_width, Hd = w.hidden;
  const bool save = a.flags & DEVIT_BLK_SAVE;
  const int t16 = w.dtype16;
  const bool drop = d && d->thr > 0;
  void* const* b = a.buf;
  TRY(zero_pad(c, b[DEVIT_ACT_LN2], D, 2));
  TRY(zero_pad(c, b[DEVIT_ACT_H], Hd, 2));
  if (save) TRY(zero_pad(c, b[DEVIT_ACT_H_PRE], Hd, 2));
  if (drop) {      // proj stores fp32 into the temporary; the residual + DropPath statement runs with the mask in it (site 2)
    devit_epilogue ep = make_ep(DEVIT_EPI_STORE_F32, d->tmp, D, c.M);
    ep.bias = w.proj_b;
    TRY(linear_fwd(c, b[DEVIT_ACT_ATTN_O], w.proj_w16, D, Da, ep));
    TRY(devit_dropout_residual(x, d->tmp, (float*)b[DEVIT_ACT_X1], a.dp1, c.N, c.M, D, d->seed, 2, d->block, d->thr, d->scale_keep, c.stream));
  } else {
    devit_epilogue ep = make_ep(DEVIT_EPI_RESIDUAL_F32, b[DEVIT_ACT_X1], D, c.M, t16);
    ep.bias = w.proj_b;
    ep.res = x;
    ep.rowscale = a.dp1;
    ep.rows_per_scale = c.N;
    ep.aux = (a.flags & DEVIT_BLK_ATT) ? b[DEVIT_ACT_ATT] : nullptr;
    TRY(linear_fwd(c, b[DEVIT_ACT_ATTN_O], w.proj_w16, D, Da, ep));
  }
  // ---- x2 = x1 + dp2 * fc2(gate * gelu(fc1(ln2(x1))))
  TRY(devit_layernorm_fwd((const float*)b[DEVIT_ACT_X1], c.M, D, 0, 0, w.n2w, w.n2b, c.eps, b[DEVIT_ACT_LN2], nullptr,
                          save ? (float*)b[DEVIT_ACT_MEAN2] : nullptr, save ? (float*)b[DEVIT_ACT_RSTD2] : nullptr, t16, c.stream));
  {
    devit_epilogue ep = make_ep(DEVIT_EPI_GELU_BF16, b[DEVIT_ACT_H], Hd, c.M, t16);
    ep.bias = w.fc1_b;
    ep.colscale = w.neuron_gate;
    ep.aux = save ? b[DEVIT_ACT_H_PRE] : nullptr;
    TRY(linear_fwd(c, b[DEVIT_ACT_LN2], w.fc1_w16, Hd, D, ep));
  }
  if (drop) {      // Mlp.drop after GELU (site 3; commutes with the neuron gate), fc2 like proj (site 4)
    TRY(devit_dropout_apply(b[DEVIT_ACT_H], 0, c.M, Hd, Hd, Hd, d->seed, 3, d->block, d->thr, d->scale_keep, nullptr, c.stream));
    devit_epilogue ep = make_ep(DEVIT_EPI_STORE_F32, d->tmp, D, c.M);
    ep.bias = w.fc2_b;
    TRY(linear_fwd(c, b[DEVIT_ACT_H], w.fc2_w16, D, Hd, ep));
    TRY(devit_dropout_residual((const float*)b[DEVIT_ACT_X1], d->tmp, (float*)b[DEVIT_ACT_X2], a.dp2, c.N, c.M, D, d->seed, 4, d->block, d->thr,
                               d->scale_keep, c.stream));
  } else {
    devit_epilogue ep = make_ep(DEVIT_EPI_RESIDUAL_F32, b[DEVIT_ACT_X2], D, c.M, t16);
    ep.bias = w.fc2_b;
    ep.res = (const float*)b[DEVIT_ACT_X1];
    ep.rowscale = a.dp2;
    ep.rows_per_scale = c.N;
    // with a k-major copy of the weight the launch can take the full-row 256x384 kernel (gemmfr.hip: bit-identical, 126 -> ~95 us in the step)
    if (w.fc2_w16t && !t16 && devit_gemm_full_row_selected(c.Mp, D, Hd, DEVIT_EPI_RESIDUAL_F32)) {
      devit_operand A = {b[DEVIT_ACT_H], Hd, 0, 0, 0, 0}, Bo = {w.fc2_w16t, D, 1, 0, 0, 0};
      TRY(devit_gemm_bf16(&A, &Bo, c.Mp, D, Hd, 1, 1, &ep, c.stream));
    } else {
      TRY(linear_fwd(c, b[DEVIT_ACT_H], w.fc2_w16, D, Hd, ep));
    }
  }
  return DEVIT_OK;
}

// d: NULL, or the block's dropout (devit_block_dropout).  thr == 0 and thr_attn == 0 (or d == NULL) is today's sequence, launch for launch.
int block_fwd(const Ctx& c, const devit_block_weights& w, const devit_block_acts& a, const devit_block_dropout* d = nullptr) {
  const int D = c.D, Da = w.attn_width, Hd = w.hidden, H = w.num_heads;
  TRY(check_dims(c.B, c.N, D, Da, Hd));
  DEVIT_CHECK(H > 0 && Da == H * 64, DEVIT_ERR_SHAPE, "block: attn_width %d != heads %d * 64", Da, H);
  const bool save = a.flags & DEVIT_BLK_SAVE;
  const int t16 = w.dtype16;
  const bool drop = d && d->thr > 0, drop_attn = d && d->thr_attn > 0;
  DEVIT_CHECK(!(drop || drop_attn) || (t16 == 0 && d->block >= 0), DEVIT_ERR_ARG, "devit_encoder_fwd_drop: dropout runs on bf16 blocks (training)");
  DEVIT_CHECK(!drop || (d->tmp && !(a.flags & DEVIT_BLK_ATT)), DEVIT_ERR_ARG,
              "devit_encoder_fwd_drop: p > 0 needs the fp32 temporary and cannot also store the attention-branch output (DEVIT_BLK_ATT)");
  DEVIT_CHECK(t16 == 0 || (t16 == 1 && !save), DEVIT_ERR_ARG,
              "devit_encoder_fwd: dtype16 = %d; f16 is the frozen-teacher forward (no DEVIT_BLK_SAVE: the backward kernels are bf16)", t16);
  void* const* b = a.buf;
  DEVIT_CHECK(a.x && b[DEVIT_ACT_LN1] && b[DEVIT_ACT_QKV] && b[DEVIT_ACT_ATTN_O] && b[DEVIT_ACT_X1] && b[DEVIT_ACT_LN2] &&
                  b[DEVIT_ACT_H] && b[DEVIT_ACT_X2],
              DEVIT_ERR_ARG, "devit_encoder_fwd: null activation buffer");
  DEVIT_CHECK(!save || (b[DEVIT_ACT_MEAN1] && b[DEVIT_ACT_RSTD1] && b[DEVIT_ACT_LSE] && b[DEVIT_ACT_MEAN2] &&
                        b[DEVIT_ACT_RSTD2] && b[DEVIT_ACT_H_PRE]),
              DEVIT_ERR_ARG, "devit_encoder_fwd: DEVIT_BLK_SAVE needs the mean/rstd/lse/h_pre buffers");
  DEVIT_CHECK(!(a.flags & DEVIT_BLK_ATT) || b[DEVIT_ACT_ATT], DEVIT_ERR_ARG, "devit_encoder_fwd: DEVIT_BLK_ATT needs att");
  TRY(zero_pad(c, b[DEVIT_ACT_LN1], D, 2));
  TRY(zero_pad(c, b[DEVIT_ACT_QKV], 3 * Da, 2, (a.flags & DEVIT_BLK_QKV_PAD) ? qkv_pad_rows(c.N) : 0));
  TRY(zero_pad(c, b[DEVIT_ACT_ATTN_O], Da, 2));
  // ---- x1 = x + dp1 * proj(gate * attn(qkv(ln1(x))))
  TRY(devit_layernorm_fwd(a.x, c.M, D, 0, 0, w.n1w, w.n1b, c.eps, b[DEVIT_ACT_LN1], nullptr,
                          save ? (float*)b[DEVIT_ACT_MEAN1] : nullptr, save ? (float*)b[DEVIT_ACT_RSTD1] : nullptr, t16, c.stream));
  {
    devit_epilogue ep = make_ep(DEVIT_EPI_STORE_BF16, b[DEVIT_ACT_QKV], 3 * Da, c.M, t16);
    ep.bias = w.qkv_b;
    TRY(linear_fwd(c, b[DEVIT_ACT_LN1], w.qkv_w16, 3 * Da, D, ep));
  }
  if (drop_attn)
    TRY(devit_attn_fwd_drop(b[DEVIT_ACT_QKV], b[DEVIT_ACT_ATTN_O], save ? (float*)b[DEVIT_ACT_LSE] : nullptr, w.head_gate, c.B, c.N, H, 64, 0.125f,
                            d->seed, d->block, d->thr_attn, d->scale_keep_attn, c.stream));
  else
  TRY(devit_attn_fwd(b[DEVIT_ACT_QKV], b[DEVIT_ACT_ATTN_O], save ? (float*)b[DEVIT_ACT_LSE] : nullptr, w.head_gate, c.B, c.N, H,
                     64, 0.125f, t16, c.stream));
  return branch_fwd(c, w, a.x, a, d);
}

}  // namespace

extern "C" int devit_block_acts_sizes(int B, int N, int D, int Da, int Hd, int flags, size_t* sizes) {
  DEVIT_CHECK(sizes != nullptr, DEVIT_ERR_ARG, "devit_block_acts_sizes: null");
  TRY(check_dims(B, N, D, Da, Hd));
  const size_t M = (size_t)B * N, Mp = pad_rows((int)M);
  const bool save = flags & DEVIT_BLK_SAVE;
  sizes[DEVIT_ACT_LN1] = Mp * D * 2;
  sizes[DEVIT_ACT_MEAN1] = sizes[DEVIT_ACT_RSTD1] = sizes[DEVIT_ACT_MEAN2] = sizes[DEVIT_ACT_RSTD2] = save ? M * 4 : 0;
  sizes[DEVIT_ACT_QKV] = (Mp + ((flags & DEVIT_BLK_QKV_PAD) ? qkv_pad_rows(N) : 0)) * 3 * (size_t)Da * 2;
  sizes[DEVIT_ACT_ATTN_O] = Mp * Da * 2;
  sizes[DEVIT_ACT_LSE] = save ? (size_t)B * (Da / 64) * N * 4 : 0;
  sizes[DEVIT_ACT_X1] = M * D * 4;
  sizes[DEVIT_ACT_ATT] = (flags & DEVIT_BLK_ATT) ? M * D * 2 : 0;
  sizes[DEVIT_ACT_LN2] = Mp * D * 2;
  sizes[DEVIT_ACT_H] = Mp * Hd * 2;
  sizes[DEVIT_ACT_H_PRE] = save ? Mp * Hd * 2 : 0;
  sizes[DEVIT_ACT_X2] = M * D * 4;
  for (int i = 0; i < DEVIT_ACT_COUNT; ++i) sizes[i] = align256(sizes[i]);
  return DEVIT_OK;
}

extern "C" int devit_block_bwd_sizes(int B, int N, int D, int Da, int Hd, size_t* sizes) {
  DEVIT_CHECK(sizes != nullptr, DEVIT_ERR_ARG, "devit_block_bwd_sizes: null");
  TRY(check_dims(B, N, D, Da, Hd));
  const size_t M = (size_t)B * N, Mp = pad_rows((int)M);
  sizes[DEVIT_BWD_DH_PRE] = Mp * Hd * 2;
  sizes[DEVIT_BWD_DLN2] = sizes[DEVIT_BWD_G1] = sizes[DEVIT_BWD_DLN1] = Mp * D * 2;
  sizes[DEVIT_BWD_DATTN] = Mp * (size_t)Da * 2;
  sizes[DEVIT_BWD_DX1] = M * D * 4;
  sizes[DEVIT_BWD_DQKV] = Mp * 3 * (size_t)Da * 2;
  sizes[DEVIT_BWD_LNWS] = devit_layernorm_bwd_workspace((int)M, D);
  for (int i = 0; i < DEVIT_BWD_COUNT; ++i) sizes[i] = align256(sizes[i]);
  return DEVIT_OK;
}

namespace {
int encoder_fwd(int nblocks, const devit_block_weights* w, const devit_block_acts* acts, const devit_block_dropout* drop, int B, int N, int D,
                float eps, void* stream) {
  DEVIT_CHECK(nblocks > 0 && w && acts, DEVIT_ERR_ARG, "devit_encoder_fwd: bad argument");
  Ctx c{B * N, pad_rows(B * N), B, N, D, eps, stream};
  // (the chain is checked whole before the first block is enqueued: a refused call has launched nothing)
  for (int i = 1; i < nblocks; ++i)
    DEVIT_CHECK(acts[i].x == (const float*)acts[i - 1].buf[DEVIT_ACT_X2], DEVIT_ERR_ARG,
                "devit_encoder_fwd: block %d does not read block %d's output", i, i - 1);
  for (int i = 0; i < nblocks; ++i) TRY(block_fwd(c, w[i], acts[i], drop ? drop + i : nullptr));
  return DEVIT_OK;
}
}  // namespace

extern "C" int devit_encoder_fwd(int nblocks, const devit_block_weights* w, const devit_block_acts* acts, int B, int N, int D,
                                 float eps, void* stream) {
  return encoder_fwd(nblocks, w, acts, nullptr, B, N, D, eps, stream);
}
extern "C" int devit_encoder_fwd_drop(int nblocks, const devit_block_weights* w, const devit_block_acts* acts, const devit_block_dropout* drop,
                                      int B, int N, int D, float eps, void* stream) {
  DEVIT_CHECK(drop != nullptr, DEVIT_ERR_ARG, "devit_encoder_fwd_drop: null dropout array");
  return encoder_fwd(nblocks, w, acts, drop, B, N, D, eps, stream);
}

namespace {
// The weight-gradient launches of one backward call.  Jobs of the grouped full-row launch where `wmode` and the shapes allow (D == 384), else --
// and for a product whose bias gradient must come from its B side (the top block's fc2) -- the split-K launch on 128x128 tiles, behind the
// kernel that produces its operand.  With a side stream (sd != NULL) each launch goes there, behind an event of that kernel on the caller's
// stream, and join() makes the caller's stream wait for them: callers see ONE stream.  They depend on nothing downstream, and beside the dgrad
// chain their workgroups fill its kernels' partial last rounds (the N = 384 dgrads run 2.32 rounds of 512 workgroups): 10233 -> 10323 img/s,
// three interleaved pairs on one box (profiles/r04_h_wgrad_side_stream_ab.txt).  DEVIT_WGRAD_STREAM=0 keeps them on the caller's stream.
struct Wgrads {
  const Ctx& c;
  WgradSide* const sd;
  const int wmode;
  devit_wgrad_job* const defer_jobs;      // the caller launches the jobs later, with other blocks' (devit_block_bwd_io.defer_jobs)
  int* const defer_count;
  Ctx cs;
  bool forked = false;
  devit_wgrad_job jobs[4];
  int nj = 0;

  Wgrads(const Ctx& c_, WgradSide* sd_, int wmode_, devit_wgrad_job* defer_jobs_, int* defer_count_)
      : c(c_), sd(sd_), wmode(wmode_), defer_jobs(defer_jobs_), defer_count(defer_count_), cs(c_) {
    if (defer_count) *defer_count = 0;
  }
  int fork(int i) {
    if (!sd) return DEVIT_OK;
    DEVIT_CHECK(hipEventRecord(sd->ev[i], (hipStream_t)c.stream) == hipSuccess && hipStreamWaitEvent(sd->stream, sd->ev[i], 0) == hipSuccess,
                DEVIT_ERR_LAUNCH, "devit_block_bwd: cannot fork the weight-gradient stream");
    cs.stream = sd->stream;
    forked = true;
    return DEVIT_OK;
  }
  int add(int ev, const void* dy, const void* x, float* w_grad, float* b_grad, int Nw, int K) {
    if (wmode && wgrad_job(&jobs[nj], dy, x, w_grad, b_grad, Nw, K)) {
      ++nj;
      return DEVIT_OK;
    }
    TRY(fork(ev));
    return linear_wgrad(cs, dy, x, w_grad, b_grad, Nw, K);
  }
  int flush(int ev) {
    if (defer_jobs) {
      for (int i = 0; i < nj; ++i) defer_jobs[i] = jobs[i];
      if (defer_count) *defer_count = nj;
      nj = 0;
      return DEVIT_OK;
    }
    if (nj == 0) return DEVIT_OK;
    TRY(fork(ev));
    const int n = nj;
    nj = 0;
    return devit_wgrad_grouped(jobs, n, c.Mp, 0, cs.stream);
  }
  // rc: what the call's launches returned.  Also behind an error after a fork: the caller's stream never runs ahead of launches it does not know about
  int join(int rc) {
    if (sd && forked) {
      const bool joined = hipEventRecord(sd->ev[4], sd->stream) == hipSuccess && hipStreamWaitEvent((hipStream_t)c.stream, sd->ev[4], 0) == hipSuccess;
      if (rc == DEVIT_OK) DEVIT_CHECK(joined, DEVIT_ERR_LAUNCH, "devit_block_bwd: cannot join the weight-gradient stream");
    }
    return rc;
  }
};

// The branch half of the backward, up to proj's dgrad and weight gradient: from dx = d loss / d x2 and g2 = bf16(dp2 * dx) to dx1 = d loss / d x1
// (ws[DEVIT_BWD_DX1]) and dattn = d loss / d attn_o (ws[DEVIT_BWD_DATTN]), on the c.M rows of a's buffers, c.N rows per DropPath scale.  ws: the
// DEVIT_BWD_* transients DH_PRE, DLN2, DX1, G1, DATTN and LNWS.  block_bwd runs it on all rows, tail_bwd on the token rows.
int branch_bwd(const Ctx& c, const devit_block_weights& w, const devit_block_acts& a, const devit_block_wgrads& g, const float* dx, const void* g2,
               bool g2_bias_done, void* const* ws, size_t lnws_bytes, const devit_block_dropout* d, Wgrads& wg) {
  const int D = c.D, Hd = w.hidden, Da = w.attn_width;
  const bool drop = d && d->thr > 0;
  void* const* b = a.buf;
  void* dh_pre = ws[DEVIT_BWD_DH_PRE];
  void* dln2 = ws[DEVIT_BWD_DLN2];
  float* dx1 = (float*)ws[DEVIT_BWD_DX1];
  void* g1 = ws[DEVIT_BWD_G1];
  void* dattn = ws[DEVIT_BWD_DATTN];
  TRY(zero_pad(c, dh_pre, Hd, 2));
  TRY(zero_pad(c, dln2, D, 2));
  TRY(zero_pad(c, g1, D, 2));
  TRY(zero_pad(c, dattn, Da, 2));
  // ---- MLP branch: x2 = x1 + dp2 * fc2(gate * gelu(fc1(ln2))).  The weight gradient that only needs g2 first, then
  // dh_pre's producer and its consumers back to back (dh_pre is 156 MB at B = 256: keep it in the Infinity Cache)
  // fc2's product is taken transposed (its 384 outputs are the B side): its bias gradient cannot come out of the grouped kernel.  Every block but the
  // topmost got it from the LN1 backward of the block above; the topmost takes a column-sum pass over g2 (the LayerNorm workspace is idle here).
  bool fc2_bias_here = !g2_bias_done;
  if (drop) {    // site 4: the incoming branch gradient is masked in place; its column sums are fc2's bias gradient
    TRY(devit_dropout_apply(const_cast<void*>(g2), 0, c.M, D, D, D, d->seed, 4, d->block, d->thr, d->scale_keep, g.fc2_b, c.stream));
    fc2_bias_here = false;
  }
  if (fc2_bias_here && wg.wmode && Hd % 128 == 0 && lnws_bytes >= devit_colsum_workspace(c.Mp, D)) {
    TRY(devit_colsum_bf16(g2, c.Mp, D, D, 0, 0, g.fc2_b, 1, ws[DEVIT_BWD_LNWS], lnws_bytes, c.stream));
    fc2_bias_here = false;
  }
  TRY(wg.add(0, g2, b[DEVIT_ACT_H], g.fc2_w, fc2_bias_here ? g.fc2_b : nullptr, D, Hd));
  {
    devit_epilogue ep = make_ep(DEVIT_EPI_DGELU_BF16, dh_pre, Hd, c.M);
    ep.colscale = w.neuron_gate;
    ep.aux_in = b[DEVIT_ACT_H_PRE];
    TRY(linear_dgrad(c, g2, w.fc2_w16, D, Hd, ep));
  }
  if (drop) TRY(devit_dropout_apply(dh_pre, 0, c.M, Hd, Hd, Hd, d->seed, 3, d->block, d->thr, d->scale_keep, nullptr, c.stream));   // site 3
  float* const g1_colsum = drop ? nullptr : g.proj_b;      // p > 0: proj's bias gradient comes from the MASKED g1 below
  // fc1's dgrad and the LN2 backward behind it: dln2 = dh_pre @ fc1_w; dx1 = dx + LN'(dln2); g1 = bf16(dp1 * dx1); its column sums = the proj bias
  // gradient.  One kernel where the full-row GEMM holds whole rows of dln2 (devit_dgrad_layernorm_bwd_fused; dln2 then never goes to memory),
  // else the two launches with the weight gradient's fork between them, as before.
  if (devit_dgrad_layernorm_bwd_fused(c.Mp, D, Hd)) {
    TRY(devit_dgrad_layernorm_bwd(dh_pre, w.fc1_w16, c.Mp, Hd, dln2, (const float*)b[DEVIT_ACT_X1], c.M, D, (const float*)b[DEVIT_ACT_MEAN2],
                                  (const float*)b[DEVIT_ACT_RSTD2], w.n2w, dx, dx1, g1, a.dp1, c.N, g.n2w, g.n2b, g1_colsum, 1,
                                  ws[DEVIT_BWD_LNWS], lnws_bytes, c.stream));
    TRY(wg.add(1, dh_pre, b[DEVIT_ACT_LN2], g.fc1_w, g.fc1_b, Hd, D));
  } else {
    TRY(linear_dgrad(c, dh_pre, w.fc1_w16, Hd, D, make_ep(DEVIT_EPI_STORE_BF16, dln2, D, c.M)));
    TRY(wg.add(1, dh_pre, b[DEVIT_ACT_LN2], g.fc1_w, g.fc1_b, Hd, D));
    TRY(devit_layernorm_bwd(dln2, 0, (const float*)b[DEVIT_ACT_X1], c.M, D, 0, 0, (const float*)b[DEVIT_ACT_MEAN2],
                            (const float*)b[DEVIT_ACT_RSTD2], w.n2w, dx, dx1, g1, a.dp1, c.N, g.n2w, g.n2b, g1_colsum, 1,
                            ws[DEVIT_BWD_LNWS], lnws_bytes, c.stream));
  }
  if (drop) TRY(devit_dropout_apply(g1, 0, c.M, D, D, D, d->seed, 2, d->block, d->thr, d->scale_keep, g.proj_b, c.stream));          // site 2
  // ---- attention branch: x1 = x + dp1 * proj(gate * attn(qkv(ln1)))
  TRY(linear_dgrad(c, g1, w.proj_w16, D, Da, make_ep(DEVIT_EPI_STORE_BF16, dattn, Da, c.M)));
  return wg.add(2, g1, b[DEVIT_ACT_ATTN_O], g.proj_w, nullptr, D, Da);
}

// (the backward checks the block and the lean last block share, in front of the first launch)
int check_bwd(const char* who, const devit_block_weights& w, const devit_block_acts& a, const devit_block_wgrads& g, int B, int N, int D) {
  const int Hd = w.hidden, H = w.num_heads, Da = w.attn_width;   // Da = H * 64 (< D when heads were compacted away)
  TRY(check_dims(B, N, D, Da, Hd));
  DEVIT_CHECK(H > 0 && Da == H * 64, DEVIT_ERR_SHAPE, "%s: attn_width %d != heads %d * 64", who, Da, H);
  DEVIT_CHECK(a.flags & DEVIT_BLK_SAVE, DEVIT_ERR_ARG, "%s: the forward ran without DEVIT_BLK_SAVE", who);
  DEVIT_CHECK(w.dtype16 == 0, DEVIT_ERR_ARG, "%s: f16 blocks have no backward", who);
  DEVIT_CHECK(g.n1w && g.n1b && g.qkv_w && g.qkv_b && g.proj_w && g.proj_b && g.n2w && g.n2b && g.fc1_w && g.fc1_b &&
                  g.fc2_w && g.fc2_b, DEVIT_ERR_ARG, "%s: null gradient accumulator", who);
  return DEVIT_OK;
}

int block_bwd(const devit_block_weights* wp, const devit_block_acts* ap, const devit_block_wgrads* gp, const devit_block_bwd_io* io,
              const devit_block_dropout* d, int B, int N, int D, float eps, void* stream) {
  DEVIT_CHECK(wp && ap && gp && io, DEVIT_ERR_ARG, "devit_block_bwd: null argument");
  const bool drop_attn = d && d->thr_attn > 0;
  DEVIT_CHECK(!(d && d->thr > 0) || !io->g2_bias_done, DEVIT_ERR_ARG,
              "devit_block_bwd_drop: with p > 0 a block forms its own fc2 bias gradient from its masked g2 (g2_bias_done must be 0)");
  // (refused here, in front of the first launch: the dropout kernels' own check of `block` would stop a backward that is half enqueued)
  DEVIT_CHECK(!((d && d->thr > 0) || drop_attn) || d->block >= 0, DEVIT_ERR_ARG, "devit_block_bwd_drop: block %d (the block's index in the model, >= 0)", d->block);
  const devit_block_weights& w = *wp;
  const devit_block_acts& a = *ap;
  const devit_block_wgrads& g = *gp;
  const int H = w.num_heads, Da = w.attn_width;
  TRY(check_bwd("devit_block_bwd", w, a, g, B, N, D));
  DEVIT_CHECK(io->dx && io->g2 && io->dx_in, DEVIT_ERR_ARG, "devit_block_bwd: dx / g2 / dx_in");
  for (int i = 0; i < DEVIT_BWD_COUNT; ++i) DEVIT_CHECK(io->ws[i], DEVIT_ERR_ARG, "devit_block_bwd: workspace %d is null", i);
  Ctx c{B * N, pad_rows(B * N), B, N, D, eps, stream};
  WgradSide* sd = nullptr;
  TRY(wgrad_side(&sd));
  Wgrads wg(c, sd, wgrad_mode(c), io->defer_jobs, io->defer_count);
  // (the body is a lambda so that an error return after a fork still joins the side stream)
  return wg.join([&]() -> int {
  void* const* b = a.buf;
  float* dx1 = (float*)io->ws[DEVIT_BWD_DX1];
  void* dattn = io->ws[DEVIT_BWD_DATTN];
  void* dqkv = io->ws[DEVIT_BWD_DQKV];
  void* dln1 = io->ws[DEVIT_BWD_DLN1];
  TRY(branch_bwd(c, w, a, g, io->dx, io->g2, io->g2_bias_done != 0, io->ws, io->lnws_bytes, d, wg));
  TRY(zero_pad(c, dqkv, 3 * Da, 2));
  TRY(zero_pad(c, dln1, D, 2));
  TRY(zero_pad(c, io->g_prev, D, 2));
  if (drop_attn)
    TRY(devit_attn_bwd_drop(b[DEVIT_ACT_QKV], b[DEVIT_ACT_ATTN_O], dattn, (const float*)b[DEVIT_ACT_LSE], w.head_gate, io->dqkv_add, dqkv, B, N, H, 64,
                            0.125f, d->seed, d->block, d->thr_attn, d->scale_keep_attn, stream));
  else
  TRY(devit_attn_bwd(b[DEVIT_ACT_QKV], b[DEVIT_ACT_ATTN_O], dattn, (const float*)b[DEVIT_ACT_LSE], w.head_gate, io->dqkv_add,
                     dqkv, B, N, H, 64, 0.125f, stream));
  // qkv's dgrad and the LN1 backward behind it, fused under the same rule: dln1 = dqkv @ qkv_w; dx_in = dx1 + LN'(dln1);
  // g_prev = bf16(prev_dp2 * dx_in) (+ the block below's fc2 bias gradient)
  if (devit_dgrad_layernorm_bwd_fused(c.Mp, D, 3 * Da)) {
    TRY(devit_dgrad_layernorm_bwd(dqkv, w.qkv_w16, c.Mp, 3 * Da, dln1, a.x, c.M, D, (const float*)b[DEVIT_ACT_MEAN1],
                                  (const float*)b[DEVIT_ACT_RSTD1], w.n1w, dx1, io->dx_in, io->g_prev, io->prev_dp2, N, g.n1w, g.n1b,
                                  io->g_prev ? io->prev_fc2_b_grad : nullptr, 1, io->ws[DEVIT_BWD_LNWS], io->lnws_bytes, stream));
    TRY(wg.add(3, dqkv, b[DEVIT_ACT_LN1], g.qkv_w, g.qkv_b, 3 * Da, D));
    TRY(wg.flush(3));
  } else {
    TRY(linear_dgrad(c, dqkv, w.qkv_w16, 3 * Da, D, make_ep(DEVIT_EPI_STORE_BF16, dln1, D, c.M)));
    TRY(wg.add(3, dqkv, b[DEVIT_ACT_LN1], g.qkv_w, g.qkv_b, 3 * Da, D));
    TRY(wg.flush(3));
    TRY(devit_layernorm_bwd(dln1, 0, a.x, c.M, D, 0, 0, (const float*)b[DEVIT_ACT_MEAN1], (const float*)b[DEVIT_ACT_RSTD1],
                            w.n1w, dx1, io->dx_in, io->g_prev, io->prev_dp2, N, g.n1w, g.n1b,
                            io->g_prev ? io->prev_fc2_b_grad : nullptr, 1, io->ws[DEVIT_BWD_LNWS], io->lnws_bytes, stream));
  }
  return DEVIT_OK;
  }());
}
}  // namespace

extern "C" int devit_block_bwd(const devit_block_weights* wp, const devit_block_acts* ap, const devit_block_wgrads* gp,
                               const devit_block_bwd_io* io, int B, int N, int D, float eps, void* stream) {
  return block_bwd(wp, ap, gp, io, nullptr, B, N, D, eps, stream);
}
extern "C" int devit_block_bwd_drop(const devit_block_weights* wp, const devit_block_acts* ap, const devit_block_wgrads* gp,
                                    const devit_block_bwd_io* io, const devit_block_dropout* drop, int B, int N, int D, float eps, void* stream) {
  DEVIT_CHECK(drop != nullptr, DEVIT_ERR_ARG, "devit_block_bwd_drop: null dropout");
  return block_bwd(wp, ap, gp, io, drop, B, N, D, eps, stream);
}

// ---- the lean last block (devit_tail_fwd / devit_tail_bwd): only the first ntok rows of every image of its output are read.  K and V are needed
// on all M = B N rows; Q, attention and the whole branch half run on the T = B ntok token rows.  Same kernels and per-row arithmetic as the block.
extern "C" int devit_tail_acts_sizes(int B, int N, int ntok, int D, int Da, int Hd, int flags, size_t* sizes) {
  DEVIT_CHECK(sizes != nullptr, DEVIT_ERR_ARG, "devit_tail_acts_sizes: null");
  TRY(check_dims(B, N, D, Da, Hd));
  DEVIT_CHECK(ntok > 0 && ntok <= N, DEVIT_ERR_SHAPE, "devit_tail_acts_sizes: ntok=%d of N=%d", ntok, N);
  const size_t M = (size_t)B * N, Mp = pad_rows((int)M), T = (size_t)B * ntok, Tp = pad_rows((int)T);
  const bool save = flags & DEVIT_BLK_SAVE;
  sizes[DEVIT_ACT_LN1] = Mp * D * 2;
  sizes[DEVIT_ACT_MEAN1] = sizes[DEVIT_ACT_RSTD1] = save ? M * 4 : 0;
  sizes[DEVIT_ACT_QKV] = Mp * 2 * (size_t)Da * 2;
  sizes[DEVIT_ACT_ATTN_O] = sizes[DEVIT_TAIL_Q] = Tp * Da * 2;
  sizes[DEVIT_ACT_LSE] = save ? (size_t)B * (Da / 64) * ntok * 4 : 0;
  sizes[DEVIT_ACT_X1] = sizes[DEVIT_ACT_X2] = sizes[DEVIT_TAIL_X_TOK] = T * D * 4;
  sizes[DEVIT_ACT_ATT] = 0;
  sizes[DEVIT_ACT_LN2] = sizes[DEVIT_TAIL_LN1_TOK] = Tp * D * 2;
  sizes[DEVIT_ACT_MEAN2] = sizes[DEVIT_ACT_RSTD2] = save ? T * 4 : 0;
  sizes[DEVIT_ACT_H] = Tp * Hd * 2;
  sizes[DEVIT_ACT_H_PRE] = save ? Tp * Hd * 2 : 0;
  for (int i = 0; i < DEVIT_TAIL_ACT_COUNT; ++i) sizes[i] = align256(sizes[i]);
  return DEVIT_OK;
}

extern "C" int devit_tail_bwd_sizes(int B, int N, int ntok, int D, int Da, int Hd, size_t* sizes) {
  DEVIT_CHECK(sizes != nullptr, DEVIT_ERR_ARG, "devit_tail_bwd_sizes: null");
  TRY(check_dims(B, N, D, Da, Hd));
  DEVIT_CHECK(ntok > 0 && ntok <= N, DEVIT_ERR_SHAPE, "devit_tail_bwd_sizes: ntok=%d of N=%d", ntok, N);
  const size_t M = (size_t)B * N, Mp = pad_rows((int)M), T = (size_t)B * ntok, Tp = pad_rows((int)T);
  sizes[DEVIT_BWD_DH_PRE] = Tp * Hd * 2;
  sizes[DEVIT_BWD_DLN2] = sizes[DEVIT_BWD_G1] = sizes[DEVIT_TAIL_BWD_DLN1_TOK] = Tp * D * 2;
  sizes[DEVIT_BWD_DATTN] = Tp * (size_t)Da * 2;
  sizes[DEVIT_BWD_DX1] = T * D * 4;
  sizes[DEVIT_BWD_DQKV] = Tp * 3 * (size_t)Da * 2;
  sizes[DEVIT_BWD_DLN1] = Mp * D * 2;
  sizes[DEVIT_BWD_LNWS] = devit_layernorm_bwd_workspace((int)M, D);
  sizes[DEVIT_TAIL_BWD_DKV] = Mp * 2 * (size_t)Da * 2;
  for (int i = 0; i < DEVIT_TAIL_BWD_COUNT; ++i) sizes[i] = align256(sizes[i]);
  return DEVIT_OK;
}

extern "C" int devit_tail_fwd(const devit_block_weights* wp, const devit_tail_acts* tp, int B, int N, int D, float eps, void* stream) {
  DEVIT_CHECK(wp && tp, DEVIT_ERR_ARG, "devit_tail_fwd: null argument");
  const devit_block_weights& w = *wp;
  const devit_block_acts& a = tp->acts;
  const int Da = w.attn_width, Hd = w.hidden, H = w.num_heads, ntok = tp->ntok, t16 = w.dtype16;
  TRY(check_dims(B, N, D, Da, Hd));
  DEVIT_CHECK(H > 0 && Da == H * 64, DEVIT_ERR_SHAPE, "devit_tail_fwd: attn_width %d != heads %d * 64", Da, H);
  DEVIT_CHECK(ntok > 0 && ntok <= N, DEVIT_ERR_SHAPE, "devit_tail_fwd: ntok=%d of N=%d", ntok, N);
  const bool save = a.flags & DEVIT_BLK_SAVE;
  DEVIT_CHECK(!(a.flags & ~DEVIT_BLK_SAVE), DEVIT_ERR_ARG, "devit_tail_fwd: flags %d (DEVIT_BLK_SAVE is the only one the lean block takes)", a.flags);
  DEVIT_CHECK(t16 == 0 || (t16 == 1 && !save), DEVIT_ERR_ARG,
              "devit_tail_fwd: dtype16 = %d; f16 is the frozen-teacher forward (no DEVIT_BLK_SAVE: the backward kernels are bf16)", t16);
  void* const* b = a.buf;
  DEVIT_CHECK(a.x && b[DEVIT_ACT_LN1] && b[DEVIT_ACT_QKV] && b[DEVIT_ACT_ATTN_O] && b[DEVIT_ACT_X1] && b[DEVIT_ACT_LN2] && b[DEVIT_ACT_H] &&
                  b[DEVIT_ACT_X2] && tp->ln1_tok && tp->q && tp->x_tok,
              DEVIT_ERR_ARG, "devit_tail_fwd: null activation buffer");
  DEVIT_CHECK(!save || (b[DEVIT_ACT_MEAN1] && b[DEVIT_ACT_RSTD1] && b[DEVIT_ACT_LSE] && b[DEVIT_ACT_MEAN2] && b[DEVIT_ACT_RSTD2] &&
                        b[DEVIT_ACT_H_PRE]),
              DEVIT_ERR_ARG, "devit_tail_fwd: DEVIT_BLK_SAVE needs the mean/rstd/lse/h_pre buffers");
  const Ctx cm{B * N, pad_rows(B * N), B, N, D, eps, stream}, ct{B * ntok, pad_rows(B * ntok), B, ntok, D, eps, stream};
  void* kv = b[DEVIT_ACT_QKV];         // (K | V) of every row: [Mp][2 Da]
  TRY(zero_pad(cm, b[DEVIT_ACT_LN1], D, 2));
  TRY(zero_pad(cm, kv, 2 * Da, 2));
  TRY(zero_pad(ct, tp->ln1_tok, D, 2));
  TRY(zero_pad(ct, tp->q, Da, 2));
  TRY(zero_pad(ct, b[DEVIT_ACT_ATTN_O], Da, 2));
  TRY(devit_layernorm_fwd(a.x, cm.M, D, 0, 0, w.n1w, w.n1b, eps, b[DEVIT_ACT_LN1], nullptr, save ? (float*)b[DEVIT_ACT_MEAN1] : nullptr,
                          save ? (float*)b[DEVIT_ACT_RSTD1] : nullptr, t16, stream));
  {
    devit_epilogue ep = make_ep(DEVIT_EPI_STORE_BF16, kv, 2 * Da, cm.M, t16);
    ep.bias = w.qkv_b + Da;
    TRY(linear_fwd(cm, b[DEVIT_ACT_LN1], (const char*)w.qkv_w16 + (size_t)Da * D * 2, 2 * Da, D, ep));
  }
  TRY(devit_token_rows_copy(b[DEVIT_ACT_LN1], N, D, tp->ln1_tok, ntok, D, B, ntok, D, 2, 0, stream));
  {
    devit_epilogue ep = make_ep(DEVIT_EPI_STORE_BF16, tp->q, Da, ct.M, t16);
    ep.bias = w.qkv_b;
    TRY(linear_fwd(ct, tp->ln1_tok, w.qkv_w16, Da, D, ep));
  }
  TRY(devit_attn_fwd_rows(tp->q, Da, kv, 2 * Da, b[DEVIT_ACT_ATTN_O], save ? (float*)b[DEVIT_ACT_LSE] : nullptr, w.head_gate, B, ntok, N, H, 64,
                          0.125f, t16, stream));
  TRY(devit_token_rows_copy(a.x, N, D, tp->x_tok, ntok, D, B, ntok, D, 4, 0, stream));
  return branch_fwd(ct, w, tp->x_tok, a, nullptr);
}

extern "C" int devit_tail_bwd(const devit_block_weights* wp, const devit_tail_acts* tp, const devit_block_wgrads* gp, const devit_tail_bwd_io* io,
                              int B, int N, int D, float eps, void* stream) {
  DEVIT_CHECK(wp && tp && gp && io, DEVIT_ERR_ARG, "devit_tail_bwd: null argument");
  const devit_block_weights& w = *wp;
  const devit_block_acts& a = tp->acts;
  const devit_block_wgrads& g = *gp;
  const int Da = w.attn_width, H = w.num_heads, ntok = tp->ntok;
  TRY(check_bwd("devit_tail_bwd", w, a, g, B, N, D));
  DEVIT_CHECK(ntok > 0 && ntok <= N, DEVIT_ERR_SHAPE, "devit_tail_bwd: ntok=%d of N=%d", ntok, N);
  DEVIT_CHECK(io->dx && io->g2 && io->dx_in, DEVIT_ERR_ARG, "devit_tail_bwd: dx / g2 / dx_in");
  for (int i = 0; i < DEVIT_TAIL_BWD_COUNT; ++i) DEVIT_CHECK(io->ws[i], DEVIT_ERR_ARG, "devit_tail_bwd: workspace %d is null", i);
  const Ctx cm{B * N, pad_rows(B * N), B, N, D, eps, stream}, ct{B * ntok, pad_rows(B * ntok), B, ntok, D, eps, stream};
  // the token-row products: split-K launches on `stream` (no jobs, no side stream: they are four small launches)
  Wgrads wg(ct, nullptr, 0, nullptr, nullptr);
  if (io->defer_count) *io->defer_count = 0;
  void* const* b = a.buf;
  void* kv = b[DEVIT_ACT_QKV];
  float* dx1 = (float*)io->ws[DEVIT_BWD_DX1];
  void* dqkv = io->ws[DEVIT_BWD_DQKV];                  // (dQ | dK | dV) of the token rows
  void* dln1 = io->ws[DEVIT_BWD_DLN1];                  // all rows
  void* dkv = io->ws[DEVIT_TAIL_BWD_DKV];               // (dK | dV) of every row
  void* dln1_tok = io->ws[DEVIT_TAIL_BWD_DLN1_TOK];
  const void* kv_w16 = (const char*)w.qkv_w16 + (size_t)Da * D * 2;
  TRY(zero_pad(ct, io->g2, D, 2));
  TRY(branch_bwd(ct, w, a, g, io->dx, io->g2, false, io->ws, io->lnws_bytes, nullptr, wg));
  TRY(zero_pad(ct, dqkv, 3 * Da, 2));
  TRY(zero_pad(cm, dkv, 2 * Da, 2));
  TRY(zero_pad(cm, dln1, D, 2));
  TRY(zero_pad(ct, dln1_tok, D, 2));
  // dO on the token rows; dQ there, dK / dV on every row
  TRY(devit_attn_bwd_rows(tp->q, Da, kv, 2 * Da, b[DEVIT_ACT_ATTN_O], io->ws[DEVIT_BWD_DATTN], (const float*)b[DEVIT_ACT_LSE], w.head_gate, dqkv,
                          3 * Da, dkv, 2 * Da, B, ntok, N, H, 64, 0.125f, stream));
  TRY(devit_token_rows_copy(dkv, N, 2 * Da, (char*)dqkv + (size_t)Da * 2, ntok, 3 * Da, B, ntok, 2 * Da, 2, 0, stream));
  // the token rows of dln1 come from one K = 3 Da GEMM like the block's (one rounding), the other rows from the K = 2 Da GEMM over (dK | dV): the
  // same sum without its zeros
  TRY(linear_dgrad(cm, dkv, kv_w16, 2 * Da, D, make_ep(DEVIT_EPI_STORE_BF16, dln1, D, cm.M)));
  TRY(linear_dgrad(ct, dqkv, w.qkv_w16, 3 * Da, D, make_ep(DEVIT_EPI_STORE_BF16, dln1_tok, D, ct.M)));
  TRY(devit_token_rows_copy(dln1_tok, ntok, D, dln1, N, D, B, ntok, D, 2, 0, stream));
  // the one product that reduces over ALL rows, (dK | dV) against ln1: a job for the caller's grouped launch where it gives a slot, else split-K
  devit_wgrad_job job;
  if (io->defer_jobs && wgrad_mode(cm) && wgrad_job(&job, dkv, b[DEVIT_ACT_LN1], g.qkv_w + (size_t)Da * D, g.qkv_b + Da, 2 * Da, D)) {
    io->defer_jobs[0] = job;
    if (io->defer_count) *io->defer_count = 1;
  } else {
    TRY(linear_wgrad(cm, dkv, b[DEVIT_ACT_LN1], g.qkv_w + (size_t)Da * D, g.qkv_b + Da, 2 * Da, D));
  }
  TRY(linear_wgrad(ct, dqkv, tp->ln1_tok, g.qkv_w, g.qkv_b, Da, D, 3 * Da));
  TRY(devit_layernorm_bwd(dln1, 0, a.x, cm.M, D, 0, 0, (const float*)b[DEVIT_ACT_MEAN1], (const float*)b[DEVIT_ACT_RSTD1], w.n1w, nullptr,
                          io->dx_in, nullptr, nullptr, 0, g.n1w, g.n1b, nullptr, 1, io->ws[DEVIT_BWD_LNWS], io->lnws_bytes, stream));
  // the residual path exists on the token rows only
  return devit_token_rows_copy(dx1, ntok, D, io->dx_in, N, D, B, ntok, D, 4, 1, stream);
}
