/* devit_hip.h -- C ABI of libdevit_hip.so: hand-written gfx950 (MI355X) kernels for the
 * DeViT hot path (ViT block forward/backward + DEKD distillation losses).
 *
 * The reference (falcon-xu/DeViT) has no FFI: its boundary is the PyTorch module surface
 * (SURVEY.md §8b).  Each entry point below names the reference op sequence it replaces
 * (file:line in the reference tree).  INTEGRATION.md shows the ctypes binding.
 *
 * Conventions (all entry points):
 *   - plain pointers + sizes, no torch types; every pointer is a DEVICE pointer unless noted
 *   - returns 0 on success, a negative DEVIT_ERR_* otherwise; devit_last_error() has the text
 *   - never allocates/frees device memory, never synchronises, enqueues only on `stream`
 *     (a hipStream_t passed as void*; NULL = default stream); safe to capture in a hipGraph
 *   - bf16 tensors are raw uint16 storage; "f32" is IEEE float
 *   - rows = tokens: M = B * N (N = 198 tokens for distilled 224x224 models)
 */
#ifndef DEVIT_HIP_H
#define DEVIT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2 (round 6): devit_block_weights grew (fc2_w16t), devit_index_copy mode 4, devit_wgrad_grouped, devit_abi_struct_size, exported symbols
 * only (the library is built with -fvisibility=hidden).  A binding asks devit_version() AND checks its struct sizes against
 * devit_abi_struct_size() before it passes arrays of structs (devit_encoder_fwd strides by sizeof(devit_block_weights)). */
/* 3: devit_set_launch_observer. */
/* 4: the lean last block per call (devit_tail_fwd / devit_tail_bwd, their two sizes functions, devit_tail_acts, devit_tail_bwd_io) and
 * devit_token_rows_copy. */
#define DEVIT_ABI_VERSION 4
#define DEVIT_API __attribute__((visibility("default")))

enum {
  DEVIT_OK = 0,
  DEVIT_ERR_SHAPE = -1,   /* dimension not supported by the kernel's tiling */
  DEVIT_ERR_ARG = -2,     /* null pointer / bad enum / misaligned pointer */
  DEVIT_ERR_LAUNCH = -3,  /* HIP reported a launch error */
  DEVIT_ERR_DEVICE = -4   /* not a gfx950 device / no device */
};

DEVIT_API int devit_version(void);
DEVIT_API const char* devit_last_error(void); /* host string, thread-local, valid until next call */
/* 0 if device `dev` is gfx950; DEVIT_ERR_DEVICE otherwise (product path refuses to run). */
DEVIT_API int devit_check_device(int dev);
/* sizeof() of the ABI's structs as THIS library was compiled (which: 0 devit_epilogue, 1 devit_operand, 2 devit_block_weights,
 * 3 devit_block_wgrads, 4 devit_block_acts, 5 devit_block_bwd_io, 6 devit_index_job, 7 devit_wgrad_job, 8 devit_launch_info, 9 devit_block_dropout,
 * 10 devit_mix_sample, 11 devit_opt_chunk, 12 devit_tail_acts, 13 devit_tail_bwd_io, 14 devit_augment_sample, 15 devit_augment_ops; anything else: 0).  A binding
 * compares them with its own mirrors once at load time: a stale mirror of a struct that is passed as an ARRAY would otherwise be misread
 * from its second element on, with no error. */
DEVIT_API size_t devit_abi_struct_size(int which);

/* ------------------------------------------------------------------------------------------
 * Launch observer: how an instrument (bench.py's per-kernel events, tools/step_gemm_table.py) sees the launches of a step without a
 * second host program.  While the CALLING THREAD has an observer installed, each of
 *     devit_gemm_bf16, devit_layernorm_fwd / _bwd, devit_attn_fwd / _bwd / _fwd_rows / _bwd_rows / _fwd_drop / _bwd_drop, devit_wgrad_grouped,
 *     devit_dgrad_layernorm_bwd (only when it takes the fused launch: unfused it calls the GEMM and LayerNorm entry points, which report)
 * calls it twice: phase 0 just before the entry point's first kernel launch (after its argument checks: a refused call reports nothing),
 * phase 1 just after its last, with the stream those kernels go to -- from inside devit_block_bwd that is the library's weight-gradient side
 * stream where the launch went there.  devit_encoder_fwd / devit_block_bwd report nothing of their own; column sums, casts, memsets, the
 * optimizer and the losses report nothing.  The pointer is thread-local (another thread's launches never enter the callback); fn == NULL
 * removes it.  With none installed an entry point pays one thread-local load and one branch.
 * devit_launch_info carries facts of the call, no labels; fields an entry point does not list are 0.
 * ---------------------------------------------------------------------------------------- */
enum { DEVIT_HAS_Y_BF16 = 1, DEVIT_HAS_Y_F32 = 2, DEVIT_HAS_DY_F32 = 4, DEVIT_HAS_DRES = 8, DEVIT_HAS_DX = 16, DEVIT_HAS_DX_BF16 = 32,
       DEVIT_HAS_DQKV_ADD = 64 };
typedef struct {
  const char* name;        /* the entry point, e.g. "devit_gemm_bf16" */
  int a_kmajor, b_kmajor, kind, M, N, K, batch, split_k; /* GEMM; the fused dgrad + LayerNorm backward: its dgrad (M_pad, D, K; kind STORE_BF16);
                                                            devit_wgrad_grouped: K = the reduction rows (M_pad), split_k = the slices taken */
  int rows, width;         /* LayerNorm: rows, D.  Attention: B * N token rows, H * head_dim features */
  int q_rows;              /* devit_attn_*_rows: B * NQ query rows */
  int has;                 /* DEVIT_HAS_*: which optional pointers of the call are not NULL (DY_F32: dy_is_f32) */
  int njobs, a_cols;       /* devit_wgrad_grouped: jobs and the sum of their a_cols */
  double flops, bytes;     /* devit_wgrad_grouped, algorithmic: 2 K a_cols 384;  K (a_cols + 384 njobs) 2 + a_cols 384 4 */
} devit_launch_info;
typedef void (*devit_launch_observer)(void* user, int phase, void* stream, const devit_launch_info* info);
DEVIT_API int devit_set_launch_observer(devit_launch_observer fn, void* user);

/* ------------------------------------------------------------------------------------------
 * GEMM  C[M,N] = sum_k A(m,k) * B(n,k), bf16 operands, fp32 accumulate (MFMA 16x16x32).
 * Replaces every nn.Linear on the path: qkv models/de_vit.py:67, proj :82, fc1 :36, fc2 :45,
 * PatchEmbed conv-as-GEMM :258 and their autograd backward (dgrad / wgrad).
 *
 *   Operands are described by devit_operand:
 *   kmajor = 0: stored [rows][K] (k contiguous), row stride ld elements       (fwd: X[M][K], W[N][K])
 *   kmajor = 1: stored [K][rows] (row index contiguous), row stride ld         (dgrad: W as B; wgrad: both)
 *   row_group/row_skip (k-major only): physical row of reduction row r is r + skip * (r / group + 1)
 *   (0/0 = dense).  Lets the patch-embed wgrad read token rows 2..197 of every image straight from the
 *   [B,198,D] gradient.
 *   batch > 1: operand z uses ptr + z * batch_stride (elements); output uses out + z * out_batch_stride.
 *   Requirements: M % 128 == 0, N % 128 == 0, K % 64 == 0, 16-byte aligned pointers / strides.
 *   Instantiated (layout, epilogue) pairs: A,B k-contiguous: STORE_BF16/F32, GELU, RESIDUAL, PATCH; B k-major
 *   (dgrad): STORE_BF16/F32, DGELU; A and B k-major (wgrad): ATOMIC_F32, STORE_F32.  Others: DEVIT_ERR_ARG.
 *   split_k > 1 is only legal with DEVIT_EPI_ATOMIC_F32.  ep->m_valid > 0 stores only rows m < m_valid
 *   of each batch (padded per-image Grams of the relation loss).
 * ---------------------------------------------------------------------------------------- */
typedef enum {
  DEVIT_EPI_STORE_BF16 = 0, /* out_bf16 = acc + bias                                           */
  DEVIT_EPI_GELU_BF16 = 1,  /* out_bf16 = gelu(acc + bias) * colscale; aux_bf16 = acc + bias    */
                            /*   (Mlp.forward de_vit.py:36-43: fc1, exact-erf GELU, neuron gate) */
  DEVIT_EPI_RESIDUAL_F32 = 2, /* out_f32 = res_f32 + rowscale[m / rows_per_scale] * (acc + bias) */
                            /*   (Block.forward :114-115 residual + DropPath); aux_bf16 optional  */
                            /*   copy of (acc + bias) (the 'attention' output, :119)              */
  DEVIT_EPI_PATCH_F32 = 3,  /* row m=(b,t): out_f32[b*(T+tok)+tok+t] = acc + bias + pos[tok+t]    */
                            /*   (forward_features :258-264; cls/dist rows written by            */
                            /*   devit_embed_tokens)                                             */
  DEVIT_EPI_DGELU_BF16 = 4, /* out_bf16 = acc * colscale * gelu'(aux_in_bf16)  (fc2 dgrad -> dfc1) */
  DEVIT_EPI_ATOMIC_F32 = 5, /* out_f32 += acc   (atomicAdd; wgrad with split-K); aux_f32[m] += sum_k A[m][k]       */
                            /*   when aux != NULL (the bias gradient of the same Linear: A = dY^T), batch == 1   */
  DEVIT_EPI_STORE_F32 = 6   /* out_f32 = acc + bias                                             */
} devit_epilogue_kind;

typedef struct {
  int kind;                /* devit_epilogue_kind */
  void* out;               /* [M][ldc] bf16 or f32 depending on kind */
  int ldc;
  const float* bias;       /* [N] or NULL */
  const float* colscale;   /* [N] gate (GELU / DGELU) or NULL (= 1) */
  void* aux;               /* GELU: pre-activation out (bf16, ld = ldc) or NULL; RESIDUAL: bf16 copy or NULL;
                              ATOMIC: f32 [M] row sums of A, accumulated, or NULL */
  const void* aux_in;      /* DGELU: saved pre-activation [M][ldc] bf16 */
  const float* res;        /* RESIDUAL: [M][ldc] f32 input stream (may alias out) */
  const float* rowscale;   /* RESIDUAL: [M / rows_per_scale] per-sample DropPath scale or NULL */
  int rows_per_scale;      /* RESIDUAL: tokens per sample (198) */
  const float* pos;        /* PATCH: [tok + T][ldc] f32 position embedding: its row stride is the OUTPUT's ldc (= N when both are dense);
                              rows tok .. tok + T - 1 and columns 0 .. N - 1 are read */
  int patch_tokens;        /* PATCH: T = 196 */
  int extra_tokens;        /* PATCH: tok = 2 (cls + dist) or 1 */
  int exact_gelu;          /* must be 0: the fused GELU is a fitted form, |err| <= 2.6e-5 (erff() variant not built) */
  long long out_batch_stride; /* elements between consecutive batch outputs (out, aux, aux_in, res) */
  int m_valid;             /* > 0: rows m >= m_valid of each batch are not stored */
  int dtype16;             /* 16-bit type of A, B and of any 16-bit output of the launch: 0 = bf16, 1 = IEEE f16 (forward
                              layouts and epilogues only: the frozen teacher's forward, 11 significand bits instead of 8) */
} devit_epilogue;

typedef struct {
  const void* ptr;         /* bf16 */
  int ld;                  /* elements */
  int kmajor;
  int row_group, row_skip;
  long long batch_stride;  /* elements */
} devit_operand;

DEVIT_API int devit_gemm_bf16(const devit_operand* A, const devit_operand* B, int M, int N, int K, int batch, int split_k,
                    const devit_epilogue* ep, void* stream);
/* The GEMM grids are persistent: one (256x256 tile) or two (128x128) workgroups per CU that walk their share of the tiles.
 * devit_set_reserved_cus(n) makes every later launch leave n CUs (a multiple of 8: one share per XCD) free for kernels of
 * other streams -- the RCCL all-reduce of the data-parallel step (distill_sub.py:333), whose kernels could otherwise start
 * only when a GEMM ends.  Default: the DEVIT_RESERVE_CUS environment variable, else 0.  Process-wide. */
/* Would devit_gemm_bf16 run (row-major A) x (K-MAJOR B) with N outputs and this epilogue kind on the full-row 256x384 kernel (N == 384, whole
 * 256-row tiles and >= 64 of them, K >= 192; DEVIT_GEMMFR=0 / 1 in the environment forces it off / on)?  1 / 0.  The fp32 residual epilogue
 * with a k-major weight exists on that kernel only, so a caller that holds a k-major copy of a forward weight (devit_block_weights.fc2_w16t)
 * asks first. */
DEVIT_API int devit_gemm_full_row_selected(int M, int N, int K, int kind);
/* Which kernel devit_gemm_bf16 would run this call on -- its one selection rule, asked instead of restated (tests tie their shapes to the
 * instantiation they mean to reach; a retune of the rule then fails them instead of silently moving them).  Returns a DEVIT_ROUTE_*: 128x128
 * tiles, 256x256 eight-wave ping-pong tiles, the full-row 256x384 kernel or the four-wave 256x256 kernel; or the negative DEVIT_ERR_* that
 * devit_gemm_bf16 returns from its argument checks for this call.  Reads DEVIT_GEMMFR / DEVIT_GEMM4 per call and DEVIT_GEMM_FORCE once per
 * process, as the launch does.  Launches nothing, dereferences no data pointer (the pointers are checked for NULL and alignment), needs no device. */
enum { DEVIT_ROUTE_TILE128 = 1, DEVIT_ROUTE_TILE256 = 3, DEVIT_ROUTE_FULL_ROW = 4, DEVIT_ROUTE_GEMM4 = 5 };
DEVIT_API int devit_gemm_route(const devit_operand* A, const devit_operand* B, int M, int N, int K, int batch, int split_k,
                     const devit_epilogue* ep);
DEVIT_API int devit_set_reserved_cus(int n);
DEVIT_API int devit_get_reserved_cus(void);

/* ------------------------------------------------------------------------------------------
 * Deterministic mode.  Off by default (DEVIT_DETERMINISTIC=1 in the environment, read once, turns it on); process-wide, like the reserved CUs.
 * The entry points whose kernels combine partial sums by fp32 atomics in arrival order -- devit_gemm_bf16 with DEVIT_EPI_ATOMIC_F32 (tile and
 * aux row sums), devit_wgrad_grouped (tiles and a_colsum), devit_embed_bwd (dpos), devit_dropout_apply (colsum), devit_cls_distill_loss (the three
 * scalars), and devit_block_bwd[_drop] through them -- then give the same bits on every run of the same call: wherever an address has more than one
 * partial sum, the partials p_0 .. p_{S-1} (S = K slices, row strips, workgroups: the default path's counts and ranges) are written to the workspace
 * and a second kernel computes
 *     out <- fp32(out + (((p_0 + p_1) + p_2) + ... + p_{S-1}))       in fp32, left to right by slice / strip / workgroup index,
 * so that the result does not depend on what the destination held either.  Call sites do not change.  devit_block_bwd[_drop] keeps its
 * weight-gradient launches on the caller's stream in this mode (as with DEVIT_WGRAD_STREAM=0).
 * Workspace: caller-owned device memory, registered per device (the current one) with devit_set_det_workspace; NULL / 0 takes it back.  Launches
 * that use it must be ordered by the caller (one stream, or events): two of them running at once would share it.  devit_det_workspace_bytes() is
 * enough for every launch of the training step (256 MiB; a caller whose launches need more registers more).  A launch that needs more than is registered returns
 * DEVIT_ERR_ARG with a message -- devit_gemm_route reports the same -- and never falls back to the atomics.
 * devit_gemm_bf16 with DEVIT_EPI_ATOMIC_F32 and batch > 1 is refused in the mode (DEVIT_ERR_ARG) when the batches' outputs overlap
 * (out_batch_stride smaller than one output): they would add into one address in arrival order.
 * devit_set / get_deterministic and devit_det_workspace_bytes need no device. */
DEVIT_API int devit_set_deterministic(int on);      /* 0 / 1 */
DEVIT_API int devit_get_deterministic(void);
DEVIT_API size_t devit_det_workspace_bytes(void);
DEVIT_API int devit_set_det_workspace(void* ws, size_t bytes);

/* ------------------------------------------------------------------------------------------
 * Weight gradients of several nn.Linear layers as ONE launch (autograd's dW = dY^T X of models/de_vit.py:67,82,36,45, i.e. what
 * engine.py:123-127's backward() leaves in .grad): a table of jobs, each
 *     out[i][j] += sum_k a[k][i] * b[k][j]      i < a_cols, j < 384           (transposed == 0: out is [a_cols][ldc])
 *     out[j][i] += ...                                                         (transposed != 0: out is [384][ldc])
 *     a_colsum[i] += sum_k a[k][i]              (optional: the bias gradient when a = dY)
 * with both operands K-MAJOR as the step holds them ([K token rows][features] bf16, rows >= the real row count zero).  One operand must be
 * exactly 384 columns wide (the student's D; fc2's gradient is taken transposed, a = the GELU output, b = dY); a_cols % 128 == 0.
 * Kernel: 256 x 384 output tiles on the full-row tile of devit_gemm_bf16 (k-major x k-major variant, one tile and one K slice per
 * workgroup, fp32 atomics through LDS in whole 256-byte rows); every workgroup of the table runs at once, so split_k slices x tiles
 * should fill the device: split_k == 0 picks the slice count by a two-term cost model (K-steps per workgroup x rounds of workgroups + the
 * atomics of every (tile, slice): csrc/wgradfr.hip).  K % 64 == 0, K / 64 / split_k >= 3, njobs <= 48 (the four products of
 * up to twelve blocks: devit_block_bwd_io.defer_jobs collects them).
 * jobs is a HOST array (copied into the kernel arguments).
 * ---------------------------------------------------------------------------------------- */
typedef struct {
  const void* a;           /* bf16 [K][lda]; a_cols columns are read (tiles of 256; a last half tile is allowed) */
  int lda, a_cols;
  const void* b;           /* bf16 [K][ldb]; columns 0..383 are read */
  int ldb;
  float* out;              /* fp32, accumulated */
  int ldc, transposed;
  float* a_colsum;         /* fp32 [a_cols], accumulated, or NULL */
} devit_wgrad_job;
DEVIT_API int devit_wgrad_grouped(const devit_wgrad_job* jobs, int njobs, int K, int split_k, void* stream);

/* ------------------------------------------------------------------------------------------
 * LayerNorm over the fp32 residual stream.  Replaces nn.LayerNorm(D, eps=1e-6) at
 * models/de_vit.py:113 (norm1), :115 (norm2), :286 (final norm) and its backward.
 *   physical input row of logical row r: in_group > 0 ? (r / in_group) * in_stride + r % in_group : r
 *   (final norm: only the cls/dist rows are consumed, de_vit.py:288 -> in_group = 2, in_stride = 198)
 *   y_bf16 / y_f32: either may be NULL.  mean / rstd: [rows] saved for backward (may be NULL).
 *   D: a multiple of 64 up to 384 (64, 192 and 320 run the ragged variant of the same kernels), or 512, 768, 1024; any other
 *   width (448, 640, ..., > 1024) is DEVIT_ERR_SHAPE before anything is launched.
 * bwd: dx[phys row] = (dres ? dres[phys row] : 0) + LN'(dy[r]); dx_bf16 (optional) = rowscale * dx as the
 *   bf16 branch gradient consumed by the previous sub-block's dgrad / wgrad GEMMs;
 *   dgamma / dbeta [D] (accumulate != 0 adds); dx_bf16_colsum (optional) [D] (+)= column sums of dx_bf16 = the
 *   bias gradient of the Linear layer that produced the branch (saves a pass over the matrix).
 *   workspace >= devit_layernorm_bwd_workspace(rows, D).
 * ---------------------------------------------------------------------------------------- */
DEVIT_API int devit_layernorm_fwd(const float* x, int rows, int D, int in_group, int in_stride, const float* gamma,
                        const float* beta, float eps, void* y_bf16, float* y_f32, float* mean, float* rstd,
                        int dtype16 /* type of y_bf16: 0 bf16, 1 f16 */, void* stream);
DEVIT_API size_t devit_layernorm_bwd_workspace(int rows, int D);
DEVIT_API int devit_layernorm_bwd(const void* dy, int dy_is_f32, const float* x, int rows, int D, int in_group, int in_stride,
                        const float* mean, const float* rstd, const float* gamma, const float* dres, float* dx,
                        void* dx_bf16, const float* rowscale, int rows_per_scale, float* dgamma, float* dbeta,
                        float* dx_bf16_colsum, int accumulate, void* workspace, size_t workspace_bytes, void* stream);

/* A Linear layer's input gradient and the LayerNorm backward behind it as one call:
 *     dln[M_pad][D] = dy[M_pad][K] @ w[K][D]     (w = the layer's [out_features K][in_features D] weight, read k-major; bf16)
 *     devit_layernorm_bwd(dln, 0, x, rows, D, 0, 0, mean, ..., stream)
 * i.e. autograd through `fc1(norm2(x))` / `qkv(norm1(x))` of models/de_vit.py:113-116 back to the residual stream.  Where
 * devit_dgrad_layernorm_bwd_fused(M_pad, D, K) says so -- D == 384, the full-row 256x384 kernel would run the product
 * (devit_gemm_full_row_selected) and every workgroup of its grid gets at most one tile (M_pad / 256 <= CUs - reserved CUs) --
 * both run in ONE kernel: the tile's rows go through LDS instead of memory and dln is not written.  dx and dx_bf16 are bit for
 * bit what the two launches give; dgamma / dbeta / dx_bf16_colsum are summed in another (fixed) order.  Otherwise, and with
 * DEVIT_LNFUSE=0 in the environment (read per call), the two launches run.  dln: [M_pad][D] bf16 scratch either way;
 * rows <= M_pad; everything else as in devit_layernorm_bwd. */
DEVIT_API int devit_dgrad_layernorm_bwd_fused(int M_pad, int D, int K);
DEVIT_API int devit_dgrad_layernorm_bwd(const void* dy, const void* w, int M_pad, int K, void* dln, const float* x, int rows, int D,
                        const float* mean, const float* rstd, const float* gamma, const float* dres, float* dx, void* dx_bf16,
                        const float* rowscale, int rows_per_scale, float* dgamma, float* dbeta, float* dx_bf16_colsum,
                        int accumulate, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Fused attention core.  Replaces models/de_vit.py:68-79 (unbind q,k,v; q k^T * scale; softmax;
 * @ v; transpose; head-gate mul_) and its backward.
 *   qkv  : bf16 [B*N][3*H*hd], feature index j*H*hd + h*hd + e (output of the qkv GEMM, de_vit.py:67)
 *   out  : bf16 [B*N][H*hd] (post head gate == Attention.head_output, de_vit.py:77-79)
 *   lse  : f32 [B][H][N] natural-log sum-exp of the scaled scores (NULL when no backward is needed)
 *   head_gate: f32 [H] or NULL.   head_dim must be 64, N <= 208.
 * bwd: dqkv (same layout as qkv) from dout; dqkv_add (optional, same layout) is added in.
 * ---------------------------------------------------------------------------------------- */
DEVIT_API int devit_attn_fwd(const void* qkv, void* out, float* lse, const float* head_gate, int B, int N, int H, int head_dim,
                   float scale, int dtype16 /* type of qkv and out: 0 bf16, 1 f16 */, void* stream);
DEVIT_API int devit_attn_bwd(const void* qkv, const void* out, const void* dout, const float* lse, const float* head_gate,
                   const void* dqkv_add, void* dqkv, int B, int N, int H, int head_dim, float scale, void* stream);
/* The same kernels with the query side apart from the key side: NQ <= N query rows per image against all N keys.
 * Used for the LAST block when the caller consumes only the class / distillation tokens (models/de_vit.py:286-288 reads
 * x[:, 0], x[:, 1] after the final norm; engine.py:91-92 reads q/k/v of the middle block only): the other 196 query
 * rows of that block are never read, so their attention (and projection, MLP) is not computed -- same arithmetic per
 * computed row, bit-identical outputs.
 *   q   : bf16 [B*NQ][q_ld], feature h*hd + e        kv  : bf16 [B*N][kv_ld], K at feature h*hd + e, V at H*hd + h*hd + e
 *   out / dout : bf16 [B*NQ][H*hd]                    lse : f32 [B][H][NQ]
 *   dq  : bf16 [B*NQ][dq_ld]                          dkv : bf16 [B*N][dkv_ld] (dK | dV), every key row written */
DEVIT_API int devit_attn_fwd_rows(const void* q, int q_ld, const void* kv, int kv_ld, void* out, float* lse, const float* head_gate,
                        int B, int NQ, int N, int H, int head_dim, float scale, int dtype16, void* stream);
DEVIT_API int devit_attn_bwd_rows(const void* q, int q_ld, const void* kv, int kv_ld, const void* out, const void* dout,
                        const float* lse, const float* head_gate, void* dq, int dq_ld, void* dkv, int dkv_ld, int B, int NQ,
                        int N, int H, int head_dim, float scale, void* stream);

/* ------------------------------------------------------------------------------------------
 * Dropout (nn.Dropout with p > 0: models/de_vit.py:38,46 Mlp.drop, :72 attn_drop, :83 proj_drop, :173 pos_drop).  ONE mask definition,
 * counter-based and never stored -- a backward regenerates what its forward used:
 *   generator  Philox4x32-10
 *   key        (seed & 0xffffffff, seed >> 32); seed = one 64-bit value per model forward
 *   counter    (g & 0xffffffff, g >> 32, site, block), g = e >> 2, e = row * pitch + col the element's LOGICAL index, pitch % 4 == 0;
 *              element e takes output word e & 3
 *   keep       iff word >= thr, thr = min(floor(p * 2^32), 2^32 - 1) computed by the host in double precision (thr == 0 keeps everything)
 *   kept values are multiplied by scale_keep = 1 / (1 - p) in fp32
 *   site  0 pos_drop   fp32 token stream after embedding   block 0        [B*T][D]
 *         1 attn_drop  the normalised softmax P            block index    row (b*H + h)*N + q, column k, pitch = ceil4(N)
 *         2 proj_drop  proj's output                       block index    [M][D]
 *         3 Mlp.drop   after GELU                          block index    [M][hidden]
 *         4 Mlp.drop   after fc2                           block index    [M][D]
 * devit_dropout_mask     keep [rows][cols] bytes (1 = kept) of a site: a debug / test entry point on the device function every kernel uses.
 * devit_dropout_apply    in place on a bf16 (is_f32 == 0) or fp32 [rows][ld] buffer, columns 0..cols-1 of rows 0..rows-1 (pad rows are not
 *                        touched); colsum (optional, fp32 [cols]) += the column sums of the masked result as stored: a Linear's bias
 *                        gradient when the buffer is its dY.  16-byte accesses: cols and ld multiples of 8 (bf16) / 4 (fp32).
 * devit_dropout_residual x_out = x + rowscale[m / rows_per_scale] * keep * scale_keep * y on fp32 [rows][cols] (x_out may alias x; pitch =
 *                        cols): the residual + DropPath statement of DEVIT_EPI_RESIDUAL_F32 with the mask in it, for sites 2 and 4, whose
 *                        GEMMs then store y through DEVIT_EPI_STORE_F32.
 * devit_attn_fwd_drop / devit_attn_bwd_drop: devit_attn_fwd / devit_attn_bwd (bf16) with site 1 inside the kernel.  P is normalised, then
 *                        masked and scaled; lse is that of the undropped row; dV = (P keep s)^T dO, dS = P (dP keep s - delta).  With thr == 0
 *                        and scale_keep == 1 the outputs are bit for bit those of devit_attn_fwd / devit_attn_bwd.  Both report to the
 *                        launch observer under their own names.
 * ---------------------------------------------------------------------------------------- */
DEVIT_API int devit_dropout_mask(unsigned long long seed, int site, int block, unsigned thr, int rows, int cols, long long pitch,
                       unsigned char* keep, void* stream);
DEVIT_API int devit_dropout_apply(void* x, int is_f32, int rows, int cols, int ld, long long pitch, unsigned long long seed, int site,
                        int block, unsigned thr, float scale_keep, float* colsum, void* stream);
DEVIT_API int devit_dropout_residual(const float* x, const float* y, float* x_out, const float* rowscale, int rows_per_scale, int rows,
                           int cols, unsigned long long seed, int site, int block, unsigned thr, float scale_keep, void* stream);
DEVIT_API int devit_attn_fwd_drop(const void* qkv, void* out, float* lse, const float* head_gate, int B, int N, int H, int head_dim,
                        float scale, unsigned long long seed, int block, unsigned thr, float scale_keep, void* stream);
DEVIT_API int devit_attn_bwd_drop(const void* qkv, const void* out, const void* dout, const float* lse, const float* head_gate,
                        const void* dqkv_add, void* dqkv, int B, int N, int H, int head_dim, float scale, unsigned long long seed,
                        int block, unsigned thr, float scale_keep, void* stream);

/* ------------------------------------------------------------------------------------------
 * Whole encoder blocks per call.  Replaces Block.forward (models/de_vit.py:103-121: norm1 -> Attention :65-87 ->
 * DropPath + residual -> norm2 -> Mlp :35-47 -> DropPath + residual) and its autograd backward as ONE host call that
 * enqueues the block's 8 (forward) / 14 (backward) kernels -- the same kernels, arguments and order as the
 * single-kernel entry points above, so results are bit-identical to calling those one by one.  It exists to take the
 * host out of the step: a DEKD step is ~650 launches, and a Python/ctypes round trip per launch costs more than the
 * kernels take (19 ms of host time for a 28 ms step).  All memory is the caller's; nothing is allocated here.
 *
 *   devit_block_weights : device pointers of one block's parameters (bf16 GEMM copies + fp32 biases / LN params / gates)
 *   devit_block_acts    : one block forward's activations; buffer sizes from devit_block_acts_sizes (index = DEVIT_ACT_*).
 *                         bf16 row buffers have pad_rows(M) = ceil(M / 256) * 256 rows (qkv: + 128 when flagged) and
 *                         their rows >= M are zeroed by the forward (GEMM tiles read them, the weight-gradient GEMMs
 *                         reduce over them).  Pointers of buffers whose size is reported 0 may be NULL.
 *   flags               : DEVIT_BLK_SAVE   keep what backward needs (mean/rstd, lse, fc1 pre-activation)
 *                         DEVIT_BLK_QKV_PAD zeroed overhang rows behind qkv (read by the relation-loss Gram windows, 256 rows
 *                                           per image): 128 for N >= 128, 256 - N for a shorter sequence
 *                         DEVIT_BLK_ATT    also store the attention-branch output (pre-residual, de_vit.py:119) as bf16
 *   devit_encoder_fwd   : blocks 0..nblocks-1 in sequence; acts[i].x2 feeds acts[i+1].x (the caller points them at the
 *                         same memory); flags per block.
 *   devit_block_bwd     : gradient of one block.  io->dx = d loss / d x2 (fp32), io->g2 = bf16(dp2 * dx) with zero pad
 *                         rows; produces io->dx_in and (optional) io->g_prev = bf16(prev_dp2 * dx_in) for the block
 *                         below together with that block's fc2 bias gradient (column sums, io->prev_fc2_b_grad);
 *                         weight gradients are ACCUMULATED into devit_block_wgrads (fp32).  io->dqkv_add: gradient
 *                         arriving at the packed qkv output from outside the block (relation loss) or NULL.
 *                         The seven transient buffers are sized by devit_block_bwd_sizes and may be reused by the next
 *                         call; their pad rows are zeroed here.
 * ---------------------------------------------------------------------------------------- */
typedef struct {
  const float *n1w, *n1b, *qkv_b, *proj_b, *n2w, *n2b, *fc1_b, *fc2_b;
  const void *qkv_w16, *proj_w16, *fc1_w16, *fc2_w16;   /* bf16 [out][in] */
  const float *head_gate, *neuron_gate;                 /* [heads] / [hidden] or NULL (= 1) */
  int num_heads, attn_width, hidden;                    /* attn_width = heads * 64 (== D unless compacted) */
  int dtype16;                                          /* 16-bit type of the weights and of every stored activation: 0 bf16,
                                                           1 f16 (forward without DEVIT_BLK_SAVE only) */
  const void* fc2_w16t;                                 /* bf16 [hidden][D]: a k-major copy of fc2_w16 (devit_index_copy mode 4), or NULL.
                                                           With it, D == 384 and >= 64 row tiles of 256 the forward's fc2 launch runs on the
                                                           full-row 256x384 GEMM (same products, same accumulation order: bit-identical) */
} devit_block_weights;

typedef struct {
  float *n1w, *n1b, *qkv_w, *qkv_b, *proj_w, *proj_b, *n2w, *n2b, *fc1_w, *fc1_b, *fc2_w, *fc2_b;
} devit_block_wgrads;

enum { DEVIT_ACT_LN1 = 0, DEVIT_ACT_MEAN1, DEVIT_ACT_RSTD1, DEVIT_ACT_QKV, DEVIT_ACT_ATTN_O, DEVIT_ACT_LSE, DEVIT_ACT_X1,
       DEVIT_ACT_ATT, DEVIT_ACT_LN2, DEVIT_ACT_MEAN2, DEVIT_ACT_RSTD2, DEVIT_ACT_H, DEVIT_ACT_H_PRE, DEVIT_ACT_X2,
       DEVIT_ACT_COUNT };
enum { DEVIT_BLK_SAVE = 1, DEVIT_BLK_QKV_PAD = 2, DEVIT_BLK_ATT = 4 };

typedef struct {
  const float* x;          /* in: fp32 [M][D] residual stream */
  void* buf[DEVIT_ACT_COUNT];
  const float *dp1, *dp2;  /* per-sample DropPath scales [B] of the two branches or NULL */
  int flags;
} devit_block_acts;

enum { DEVIT_BWD_DH_PRE = 0, DEVIT_BWD_DLN2, DEVIT_BWD_DX1, DEVIT_BWD_G1, DEVIT_BWD_DATTN, DEVIT_BWD_DQKV, DEVIT_BWD_DLN1,
       DEVIT_BWD_LNWS, DEVIT_BWD_COUNT };

typedef struct {
  const float* dx;         /* in: fp32 [M][D] */
  const void* g2;          /* in: bf16 [pad_rows(M)][D] */
  float* dx_in;            /* out: fp32 [M][D] */
  void* g_prev;            /* out: bf16 [pad_rows(M)][D] or NULL */
  const float* prev_dp2;   /* [B] or NULL */
  float* prev_fc2_b_grad;  /* [D] accumulated, or NULL */
  int g2_bias_done;        /* != 0: this block's fc2 bias gradient was already produced by the block above */
  const void* dqkv_add;    /* bf16, qkv layout, or NULL */
  void* ws[DEVIT_BWD_COUNT];
  size_t lnws_bytes;
  devit_wgrad_job* defer_jobs; /* HOST array of >= 4 entries or NULL.  Not NULL: the block's weight gradients that can run on the full-row
                                  weight-gradient kernel are NOT launched; they are written here as jobs for a later devit_wgrad_grouped call
                                  (several blocks in one launch: fewer K slices, fewer atomics).  The caller then keeps io->g2 and the
                                  DH_PRE / G1 / DQKV transients (and the forward's activations) alive until that launch has been enqueued */
  int* defer_count;            /* out: jobs written */
} devit_block_bwd_io;

DEVIT_API int devit_block_acts_sizes(int B, int N, int D, int attn_width, int hidden, int flags, size_t* sizes /* [DEVIT_ACT_COUNT] */);
DEVIT_API int devit_block_bwd_sizes(int B, int N, int D, int attn_width, int hidden, size_t* sizes /* [DEVIT_BWD_COUNT] */);
DEVIT_API int devit_encoder_fwd(int nblocks, const devit_block_weights* w, const devit_block_acts* acts, int B, int N, int D,
                      float eps, void* stream);
/* devit_block_bwd is the ONE entry point that does not keep to "enqueue on the caller's stream only": its four weight-gradient GEMMs go to a
 * stream the LIBRARY owns -- one non-blocking stream + five events per device, created at the first call on that device (thread-safe), never
 * destroyed: process lifetime -- each behind an event of the kernel on `stream` that produces its operand, and `stream` waits for the last of them
 * before the call returns (also when it returns an error after the first fork).  Callers therefore still see one stream: everything the call
 * enqueued is ordered before whatever is enqueued on `stream` next, the transient buffers may be reused, the accumulators in `grads` are complete
 * for the next kernel on `stream`.  What a binding must know: (1) the call is not capturable into a hipGraph of `stream` alone before
 * the side stream exists (first call outside capture); (2) a stream-ordered allocator must treat the buffers of `acts` / `io` / `grads` as in use
 * until work enqueued on `stream` AFTER the call has run (they are read by another stream meanwhile); (3) DEVIT_WGRAD_STREAM=0 in the environment
 * (read per call) keeps every launch on `stream`; a device index >= 16 does the same.  Worth +0.9 % on the DEKD step (profiles/r04_h_*). */
DEVIT_API int devit_block_bwd(const devit_block_weights* w, const devit_block_acts* acts, const devit_block_wgrads* grads,
                    const devit_block_bwd_io* io, int B, int N, int D, float eps, void* stream);

/* ------------------------------------------------------------------------------------------
 * The lean last block per call: the caller reads only the first ntok rows of every image of the block's output (the class / distillation
 * tokens, models/de_vit.py:286-288).  LN1 and the K and V projections run on all M = B * N rows; the Q projection, attention
 * (devit_attn_fwd_rows) and everything from proj on -- the SAME host sequence as the block's, csrc/encoder.hip: branch_fwd / branch_bwd -- on
 * the T = B * ntok token rows, ntok rows per DropPath scale.  Same kernels and per-row arithmetic as devit_encoder_fwd, so the token rows of
 * the output are bit-identical to the block's.  All launches go to `stream`; nothing is allocated, nothing synchronises.
 *
 *   devit_tail_acts  : acts.x is the block's fp32 [M][D] input and acts.buf[] the block's buffers with these extents (sizes from
 *                      devit_tail_acts_sizes, index DEVIT_ACT_* / DEVIT_TAIL_*; Mp = pad_rows(M), Tp = pad_rows(T)):
 *                        LN1 16-bit [Mp][D], MEAN1 / RSTD1 [M]        QKV: (K | V) 16-bit [Mp][2 attn_width]
 *                        ATTN_O 16-bit [Tp][attn_width], LSE [B][heads][ntok]      X1, X2 fp32 [T][D]     LN2 16-bit [Tp][D], MEAN2 / RSTD2 [T]
 *                        H, H_PRE 16-bit [Tp][hidden]                 ATT: unused (size 0)
 *                      and what the block has no place for: ln1_tok 16-bit [Tp][D] (the token rows of LN1), q 16-bit [Tp][attn_width],
 *                      x_tok fp32 [T][D] (the token rows of x).  acts.flags: DEVIT_BLK_SAVE or 0.  The output is buf[DEVIT_ACT_X2].
 *                      Pad rows of every 16-bit row buffer are zeroed by the forward.
 *   devit_tail_bwd   : io->dx = d loss / d x2 fp32 [T][D], io->g2 = bf16(dp2 * dx) in the first T of its Tp rows; produces io->dx_in fp32 [M][D].
 *                      Transients from devit_tail_bwd_sizes (index DEVIT_BWD_* / DEVIT_TAIL_BWD_*): the block's on Tp rows -- DQKV is
 *                      (dQ | dK | dV) of the token rows -- except DLN1 [Mp][D] and LNWS (for M rows); DKV 16-bit [Mp][2 attn_width],
 *                      DLN1_TOK 16-bit [Tp][D].  Weight gradients are accumulated by split-K launches on `stream`.  io->defer_jobs (a HOST
 *                      array of >= 1 entry) not NULL: the one product that reduces over all rows, (dK | dV)^T ln1, is written there as a job
 *                      for a later devit_wgrad_grouped(..., K = Mp, ...) call where the full-row weight-gradient kernel takes it (D == 384,
 *                      DEVIT_WGRADFR not 0) instead of being launched; the caller then keeps DKV and LN1 alive until that launch.
 * ---------------------------------------------------------------------------------------- */
enum { DEVIT_TAIL_LN1_TOK = DEVIT_ACT_COUNT, DEVIT_TAIL_Q, DEVIT_TAIL_X_TOK, DEVIT_TAIL_ACT_COUNT };
typedef struct {
  devit_block_acts acts;
  void *ln1_tok, *q;
  float* x_tok;
  int ntok;                /* 0 < ntok <= N */
} devit_tail_acts;

enum { DEVIT_TAIL_BWD_DKV = DEVIT_BWD_COUNT, DEVIT_TAIL_BWD_DLN1_TOK, DEVIT_TAIL_BWD_COUNT };
typedef struct {
  const float* dx;         /* in: fp32 [T][D] */
  void* g2;                /* in: bf16 [pad_rows(T)][D]; its rows >= T are zeroed by the call */
  float* dx_in;            /* out: fp32 [M][D] */
  void* ws[DEVIT_TAIL_BWD_COUNT];
  size_t lnws_bytes;
  devit_wgrad_job* defer_jobs;
  int* defer_count;        /* out: jobs written (0 or 1) */
} devit_tail_bwd_io;

DEVIT_API int devit_tail_acts_sizes(int B, int N, int ntok, int D, int attn_width, int hidden, int flags, size_t* sizes /* [DEVIT_TAIL_ACT_COUNT] */);
DEVIT_API int devit_tail_bwd_sizes(int B, int N, int ntok, int D, int attn_width, int hidden, size_t* sizes /* [DEVIT_TAIL_BWD_COUNT] */);
DEVIT_API int devit_tail_fwd(const devit_block_weights* w, const devit_tail_acts* acts, int B, int N, int D, float eps, void* stream);
DEVIT_API int devit_tail_bwd(const devit_block_weights* w, const devit_tail_acts* acts, const devit_block_wgrads* grads,
                   const devit_tail_bwd_io* io, int B, int N, int D, float eps, void* stream);

/* The first ntok rows of every image, from one strided matrix into another (the lean last block's gathers and scatters):
 *   dst[(b * dst_rows_per_image + t) * dst_ld + c]  =  (or, add != 0, +=)  src[(b * src_rows_per_image + t) * src_ld + c],   b < B, t < ntok, c < cols
 * elem: bytes per element, 2 or 4; add needs 4 (fp32).  Leading dimensions in elements.  Moves 16-byte vectors: pointers, leading dimensions and
 * cols must be whole multiples of 16 bytes (DEVIT_ERR_ARG otherwise).  Source and destination must not overlap. */
DEVIT_API int devit_token_rows_copy(const void* src, int src_rows_per_image, int src_ld, void* dst, int dst_rows_per_image, int dst_ld, int B,
                          int ntok, int cols, int elem, int add, void* stream);

/* ------------------------------------------------------------------------------------------
 * Index copies of physically shrunk (compacted) blocks that are being TRAINED (distill_sub.py:384-401 trains the gated
 * student; core/imp_rank.py:65-71,147-153 only mask).  A table of jobs in device memory, one launch:
 *   mode 0  gather rows     dst[i][c]      = src[idx[i]][c]        (16-bit or f32 elements)
 *   mode 1  gather columns  dst[r][j]      = src[r][idx[j]]
 *   mode 2  add rows        dst[idx[i]][c] += src[i][c]            (f32: compact weight gradients into the masters'; the
 *   mode 3  add columns     dst[r][idx[j]] += src[r][j]             source is an accumulator and is ZEROED by the call)
 *   mode 4  transpose       dst[c][r]      = src[r][c]             (16-bit elements, idx unused: the k-major copy of a Linear
 *                                                                    weight the full-row GEMM reads, devit_block_weights.fc2_w16t)
 * rows x cols is the extent of the COMPACT (dense) side; idx entries < 0 mark padding units and are skipped; kept
 * indices are distinct, so the adds need no atomics.  Jobs of one call must not write the same memory.
 * ---------------------------------------------------------------------------------------- */
typedef struct {
  const void* src;
  void* dst;
  const int* idx;        /* device, rows entries (modes 0, 2) or cols entries (modes 1, 3) */
  int rows, cols;
  int src_ld, dst_ld;    /* elements */
  int mode;
  int elem;              /* bytes per element: 2 or 4 (modes 2, 3: 4) */
} devit_index_job;
DEVIT_API int devit_index_copy(const devit_index_job* jobs_device, int njobs, int blocks_per_job, void* stream);

/* ------------------------------------------------------------------------------------------
 * Unit ranking of the shrink stage (csrc/hsic.hip; core/imp_rank.py:16-47 mlp_neuron_rank, :93-129 attn_head_rank,
 * :175-239 HSICLoss).  For unit u the feature of sample a is x_a[n], n < N tokens: the mean of `group` consecutive
 * channels X[a][n][u * group ...] (group = 1: an MLP neuron of neuron_output [B][N][hidden]; group = head_dim: a head
 * of head_output [B][N][H][hd]).
 *   Kmix_u[a][b] = 1/5 sum_{s = 1, 2, 4, 8, 16} exp(-d2 / (2 s^2)),  d2 = sum_n (x_a[n] - x_b[n])^2   (fp32 differences)
 *   devit_hsic_target:     W [B][B] = center(y y^T), y = p - mean_a p, p = softmax of the rows (softmax != 0) or the rows
 *                          themselves (softmax == 0: already probabilities); workspace >= B * C floats
 *   devit_hsic_scores:     rel[u] = sum_ab Kmix_u[a][b] W[a][b];  act[u] = sum_{a, n} |X[a][n][u]| (optional, group == 1);
 *                          kmix1 [units][B][B] (optional) receives Kmix_u - 1 (zero diagonal): the sums this kernel feeds are
 *                          against centred kernels, which a constant does not enter, and on a real model Kmix lies within 1e-3
 *                          of 1 -- in fp32 the signal is kept only in this form; rel is computed from it, too (W is centred).
 *                          X: element type DEVIT_HSIC_*, channels
 *                          contiguous, batch / token strides in elements (the forward's activations are views of padded
 *                          row buffers).  workspace >= devit_hsic_scores_workspace(B, N, units) bytes, 16-byte aligned.
 *   devit_hsic_head_pairs: red[h] = 1/(H - 1) sum_{g != h} sum_ab Kmix_h[a][b] center(Kmix_g)[a][b], from kmix1 [H][B][B], H <= 16.
 * The reference's mean_sub step shifts a feature column by one constant for every sample, which the pairwise distances do
 * not see; a column that is constant and non-zero over the batch (std = 0: the reference's shift is mean * 1e12 and its
 * value cancellation noise) gets the translation-invariant value here.  2 <= B <= 256; anything else is DEVIT_ERR_ARG.
 * One workgroup owns a unit's sums: results do not depend on the launch's timing.
 * ---------------------------------------------------------------------------------------- */
enum { DEVIT_HSIC_BF16 = 0, DEVIT_HSIC_F16 = 1, DEVIT_HSIC_F32 = 2 };
DEVIT_API int devit_hsic_target(const float* y, int B, int C, int softmax, float* W, void* workspace, size_t workspace_bytes,
                      void* stream);
DEVIT_API size_t devit_hsic_scores_workspace(int B, int N, int units);
DEVIT_API int devit_hsic_scores(const void* X, int elem, int B, int N, int units, int group, long long batch_stride,
                      long long token_stride, const float* W, float* rel, float* act, float* kmix1, void* workspace,
                      size_t workspace_bytes, void* stream);
DEVIT_API int devit_hsic_head_pairs(const float* kmix1, int H, int B, float* red, void* stream);

/* ------------------------------------------------------------------------------------------
 * Patch embedding helpers (timm PatchEmbed used at models/de_vit.py:166-168,258 and token assembly
 * :259-264).  im2row: f32 [B,3,S,S] -> bf16 [B*T][768] with k = c*256 + kh*16 + kw, token t = py*G + px; the
 * projection itself is devit_gemm_bf16 with DEVIT_EPI_PATCH_F32.
 * Image sizes: C = 3, patch = 16, H == W == S with S a multiple of 16 from 32 to 224 (G = S/16 = 2 .. 14 patches per side,
 *   T = G*G tokens; 224 is the ceiling because T + 2 tokens must fit the attention kernels' 208 rows: 240 pixels are 227).
 *   Anything else is DEVIT_ERR_SHAPE.  The entry points without H, W below are the 224-pixel calls; each has a `_sized`
 *   sibling with the same arguments plus `int H, int W` in front of the stream, which at 224 is the same launch.  embed_tokens writes
 * x[b, t, :] = (t == 0 ? cls : dist) + pos[t] for the 1-2 extra tokens (dist == NULL: cls only).
 * embed_bwd: dpos[T][D] = sum_b dx[b]; dcls = dpos[0]; ddist = dpos[1]; dbias = sum_{t>=ntok} dpos[t];
 *   dx_bf16 (optional) = bf16 copy of dx for the patch-projection wgrad.
 * ---------------------------------------------------------------------------------------- */
DEVIT_API int devit_im2row_bf16(const float* img, void* rows, int B, int C, int H, int W, int patch, int dtype16, void* stream);
/* On-device input stage (engine.py:65-66: timm Mixup(mode='batch') on the fp32 batch, then patch_embed): the mixed batch is
 * produced directly as the bf16 patch rows both models' patch-embedding GEMMs read -- one pass over the images.
 *   mode 0: plain im2row; 1: mixup  lam * x + (1 - lam) * x.flip(0);  2: cutmix  x[:, :, y0:y1, x0:x1] = x.flip(0)[...]
 *   (lam, the box and the mixup / cutmix draw are host-side numpy RNG in timm; they are arguments here).
 * devit_mix_targets: [B][C] f32 = lam * smooth_one_hot(y) + (1 - lam) * smooth_one_hot(y.flip(0)), int64 labels. */
DEVIT_API int devit_mix_im2row_bf16(const float* img, void* rows /* bf16 or NULL */, void* rows_f16 /* f16 or NULL */, int B, int mode,
                          double lam, int y0, int y1, int x0, int x1, void* stream);
/* ... on [B,3,H,W] images (sizes: see above); the cutmix box is checked against H, W */
DEVIT_API int devit_mix_im2row_bf16_sized(const float* img, void* rows /* bf16 or NULL */, void* rows_f16 /* f16 or NULL */, int B, int mode,
                          double lam, int y0, int y1, int x0, int x1, int H, int W, void* stream);
DEVIT_API int devit_mix_targets(const long long* labels, float* targets, int B, int C, double lam, double smoothing, void* stream);
/* The same stage with one (mode, lam, box) PER SAMPLE (timm Mixup(mode='elem' / 'pair'), cutmix_minmax boxes): entry b of a device
 * table of B devit_mix_sample says how sample b is mixed with its partner, which is always sample B-1-b (timm's _mix_elem and
 * _mix_pair both use it; pair mode is a table with entry[b] == entry[B-1-b]).  struct id 10 of devit_abi_struct_size, 32 bytes.
 *   mode 0: sample b as it is; 1: x[b] * lam + x[B-1-b] * (1.0f - lam); 2: x[b] with [y0,y1) x [x0,x1) copied from x[B-1-b].
 * 1 - lam is computed IN FP32 from the fp32 lam, as timm's per-element path does (lam_batch is a float32 array, and 1 - lam on a
 * np.float32 stays float32).  devit_mix_im2row_bf16 / devit_mix_targets above take f32(1 - lam) with the subtraction done in
 * double by their host (torch's arithmetic with a python scalar): for a lam whose complement is not exact in fp32 the two families
 * differ in the last bit of that factor, each as its timm mode does.  The products and the sum are rounded separately.
 * devit_mix_im2row_table: any subset (not none) of three outputs -- bf16 rows, f16 rows, and img_out, the mixed batch as fp32
 *   [B,3,224,224] in image layout (for precision="f32" models).  img_out must not be img: a sample's partner is read after the
 *   sample may have been written.  B <= 65535.
 * devit_mix_targets_table: targets[b][c] = t1 * lam_b + t2 * (1.0f - lam_b), t1 / t2 the smoothed one-hot values of y[b] / y[B-1-b]
 *   (formed in double, rounded to fp32, as devit_mix_targets); lam_b is used whatever the mode, so a mode 0 entry carries lam 1.
 * No address in either kernel depends on the table's contents (only selects and branches do), so both are memory-safe for any
 * table bytes; the entries cannot be validated here without a synchronise and are the caller's to check before the upload. */
typedef struct {
  int mode;
  float lam;
  int y0, y1, x0, x1;
  int reserved[2];
} devit_mix_sample;
DEVIT_API int devit_mix_im2row_table(const float* img, void* rows /* bf16 or NULL */, void* rows_f16 /* f16 or NULL */,
                           float* img_out /* f32 images or NULL */, const devit_mix_sample* table /* device, B entries */, int B,
                           void* stream);
/* ... on [B,3,H,W] images (img_out has the same shape); the host checks the table's boxes against H, W */
DEVIT_API int devit_mix_im2row_table_sized(const float* img, void* rows /* bf16 or NULL */, void* rows_f16 /* f16 or NULL */,
                           float* img_out /* f32 images or NULL */, const devit_mix_sample* table /* device, B entries */, int B,
                           int H, int W, void* stream);
DEVIT_API int devit_mix_targets_table(const long long* labels, float* targets, const devit_mix_sample* table, int B, int C,
                            double smoothing, void* stream);
DEVIT_API int devit_embed_tokens(const float* cls, const float* dist, const float* pos, float* x, int B, int T, int D,
                       void* stream);
DEVIT_API int devit_embed_bwd(const float* dx, int B, int T, int D, int ntok, float* dpos, float* dcls, float* ddist,
                    float* dbias, void* dx_bf16, int accumulate, void* stream);

/* f32 -> bf16 cast of a flat buffer (weights, once per optimizer step). */
DEVIT_API int devit_cast_bf16(const float* src, void* dst, size_t n, int dtype16, void* stream);

/* dst_bf16[m][d] = bf16(src[m][d] * (rowscale ? rowscale[m / rows_per_scale] : 1)): turns the fp32
 * residual-stream gradient into the bf16 branch gradient (DropPath scale folded, de_vit.py:114-115). */
DEVIT_API int devit_scale_cast_bf16(const float* src, void* dst, const float* rowscale, int rows_per_scale, int M, int D,
                          void* stream);

/* Column sums of a bf16 [M][ld] matrix: out[n] (+)= sum_m y[m][n]  (bias gradients of nn.Linear).
 * row_group/row_skip as in devit_operand.  workspace >= devit_colsum_workspace(M, N). */
DEVIT_API size_t devit_colsum_workspace(int M, int N);
DEVIT_API int devit_colsum_bf16(const void* y, int M, int N, int ld, int row_group, int row_skip, float* out, int accumulate,
                      void* workspace, size_t workspace_bytes, void* stream);

/* Small strided f32 GEMM  C[m][n] (+)= alpha * sum_k A[m*sam + k*sak] * B[n*sbn + k*sbk] + bias[n].
 * Classifier heads (models/de_vit.py:317) and their backward; exact fp32 FMA chain. */
DEVIT_API int devit_sgemm_small(const float* A, long long sam, long long sak, const float* B, long long sbn, long long sbk,
                      const float* bias, float* C, int ldc, int M, int N, int K, float alpha, int accumulate,
                      void* stream);

/* ------------------------------------------------------------------------------------------
 * Optimizer tail over FLAT fp32 buffers (engine.py:127 NativeScaler -> clip_grad_norm_ -> AdamW.step,
 * engine.py:131-132 ModelEma.update): sum of squares (global grad norm), then one fused pass
 *   g *= grad_scale * min(1, max_norm / (||g|| + 1e-6));  AdamW;  ema = ema*d + (1-d)*p;  p_bf16 = bf16(p)
 * dyn = device float[3] {lr, 1 - beta1^step, 1 - beta2^step} (device-resident so a captured graph can
 * be replayed while the schedule advances).  gnorm_sq == NULL: no clipping.  n % 4 == 0.
 * no_decay4: one byte per 4-element granule of the flat buffer, non-zero = exempt from weight decay (timm
 * create_optimizer's second parameter group: 1-D tensors, biases, model.no_weight_decay(); distill_sub.py:340); NULL =
 * decay everywhere.  grad_scale: the 1 / world_size of the data-parallel mean (the buckets are all-reduced as sums).
 * ---------------------------------------------------------------------------------------- */
DEVIT_API size_t devit_sumsq_workspace(void);
DEVIT_API int devit_sumsq_f32(const float* g, size_t n, float* out, void* workspace, size_t workspace_bytes, void* stream);
DEVIT_API int devit_adamw_step(float* p, const float* g, float* m, float* v, float* ema, void* p_bf16,
                     const unsigned char* no_decay4, const float* gnorm_sq, const float* dyn, size_t n, float beta1,
                     float beta2, float eps, float weight_decay, float max_norm, float ema_decay, float grad_scale,
                     void* stream);

/* The same tail for timm's other optimizers (create_optimizer names `momentum`, `nesterov`, `adam`, `lamb`, `lambc`).  Shared with
 * devit_adamw_step, argument for argument: g' = g * clip with clip = grad_scale * min(1, max_norm / (sqrt(gnorm_sq) * grad_scale + 1e-6))
 * (gnorm_sq == NULL: clip = grad_scale), the no_decay4 granule mask (weight decay 0 there), ema = ema*d + (1-d)*p', p_bf16 = bf16(p')
 * (ema, p_bf16 optional), dyn on the device, n % 4 == 0.  Everything is fp32; wd is the granule's weight decay.
 *   devit_sgd_step      torch.optim.SGD(momentum = mu, nesterov, dampening 0); dyn = float[1] {lr}; buf starts at zero
 *                         d = g' + wd p;  buf' = mu buf + d;  p' = p - lr (nesterov ? d + mu buf' : buf')
 *   devit_adam_l2_step  torch.optim.Adam (L2 decay coupled into the gradient); dyn = float[3] as devit_adamw_step
 *                         d = g' + wd p;  m' = b1 m + (1-b1) d;  v' = b2 v + (1-b2) d d;  p' = p - (lr/bc1) m' / (sqrt(v')/sqrt(bc2) + eps)
 *   devit_lamb_step     timm Lamb (bias_correction, grad_averaging, max_grad_norm = 1, always_adapt = False); dyn = float[3]
 *                         gnorm_sq is REQUIRED; max_norm <= 0: no outer clip (clip = grad_scale)
 *                         n1 = sqrt(gnorm_sq) * clip;  g'' = g' / max(1, n1);  m' = b1 m + (1-b1) g'';  v' = b2 v + (1-b2) g'' g''
 *                         u = (m'/bc1) / (sqrt(v')/sqrt(bc2) + eps), + wd p in a decayed tensor
 *                         per decayed tensor trust = (||p|| > 0 and ||u|| > 0) ? ||p|| / ||u|| : 1, min(trust, 1) with trust_clip
 *                         (`lambc`); tensors of the no-decay group take trust = 1;  p' = p - lr trust u
 * LAMB's norms run over ONE parameter tensor, so its caller describes the flat buffer by a device table of devit_opt_chunk (struct id
 * 11 of devit_abi_struct_size, 16 bytes): chunk c covers granules [first4, first4 + count4) -- count4 <= 1024, all of tensor
 * `segment` (0 <= segment < nsegments) -- with flags bit 0 set when that tensor is exempt from weight decay.  The table is sorted by
 * segment, its chunks are disjoint, and granules that no chunk covers (padding between tensors) are left untouched.  The caller
 * validates the table before it uploads it; the kernels additionally skip a chunk that would reach outside [0, n / 4) or
 * nsegments.  Three launches (moments and per-chunk partial norms; one wave per tensor adds them in chunk order; the update with u
 * recomputed from p, m', v'), no atomics: the same input gives the same bits.  workspace >= devit_lamb_workspace(nchunks,
 * nsegments) bytes, 8-byte aligned, owned by the caller: [nchunks][2] partial sums, then trust[nsegments]. */
typedef struct {
  unsigned first4;
  unsigned count4;
  int segment;
  int flags;
} devit_opt_chunk;
DEVIT_API int devit_sgd_step(float* p, const float* g, float* buf, float* ema, void* p_bf16, const unsigned char* no_decay4,
                   const float* gnorm_sq, const float* dyn, size_t n, float momentum, int nesterov, float weight_decay,
                   float max_norm, float ema_decay, float grad_scale, void* stream);
DEVIT_API int devit_adam_l2_step(float* p, const float* g, float* m, float* v, float* ema, void* p_bf16,
                       const unsigned char* no_decay4, const float* gnorm_sq, const float* dyn, size_t n, float beta1,
                       float beta2, float eps, float weight_decay, float max_norm, float ema_decay, float grad_scale,
                       void* stream);
DEVIT_API size_t devit_lamb_workspace(int nchunks, int nsegments);
DEVIT_API int devit_lamb_step(float* p, const float* g, float* m, float* v, float* ema, void* p_bf16, const float* gnorm_sq,
                    const float* dyn, size_t n, const devit_opt_chunk* chunks, int nchunks, int nsegments, int trust_clip,
                    float beta1, float beta2, float eps, float weight_decay, float max_norm, float ema_decay, float grad_scale,
                    void* workspace, size_t workspace_bytes, void* stream);

/* The four tails with a learning rate per granule (layer-wise lr decay: lr x decay^(distance from the head)).  Each takes its sibling's
 * arguments and, in front of the stream, two more, both required:
 *   lr_group4   one byte per 4-element granule of the flat buffer, n / 4 bytes, laid out like no_decay4: the index of the granule's scale
 *   lr_scales   a device table of EXACTLY 256 floats.  Every value a byte can hold indexes inside it, so the kernels check nothing and no
 *               address depends on the contents of lr_group4; entries that no granule uses should hold 1.
 * The granule's learning rate is fp32(dyn[0]) * lr_scales[lr_group4[granule]], one fp32 multiply, and stands wherever the sibling uses lr:
 * AdamW in p *= 1 - lr wd and in the update, SGD and Adam in the update, LAMB in p' = p - lr trust u (the moments and the trust ratio do not
 * see the scale).  A table of ones gives the sibling's bits.  A scale of 0 freezes its granules' learning rate (moments and EMA still move). */
DEVIT_API int devit_adamw_step_lrs(float* p, const float* g, float* m, float* v, float* ema, void* p_bf16,
                         const unsigned char* no_decay4, const float* gnorm_sq, const float* dyn, size_t n, float beta1,
                         float beta2, float eps, float weight_decay, float max_norm, float ema_decay, float grad_scale,
                         const unsigned char* lr_group4, const float* lr_scales, void* stream);
DEVIT_API int devit_sgd_step_lrs(float* p, const float* g, float* buf, float* ema, void* p_bf16, const unsigned char* no_decay4,
                       const float* gnorm_sq, const float* dyn, size_t n, float momentum, int nesterov, float weight_decay,
                       float max_norm, float ema_decay, float grad_scale, const unsigned char* lr_group4,
                       const float* lr_scales, void* stream);
DEVIT_API int devit_adam_l2_step_lrs(float* p, const float* g, float* m, float* v, float* ema, void* p_bf16,
                           const unsigned char* no_decay4, const float* gnorm_sq, const float* dyn, size_t n, float beta1,
                           float beta2, float eps, float weight_decay, float max_norm, float ema_decay, float grad_scale,
                           const unsigned char* lr_group4, const float* lr_scales, void* stream);
DEVIT_API int devit_lamb_step_lrs(float* p, const float* g, float* m, float* v, float* ema, void* p_bf16, const float* gnorm_sq,
                        const float* dyn, size_t n, const devit_opt_chunk* chunks, int nchunks, int nsegments, int trust_clip,
                        float beta1, float beta2, float eps, float weight_decay, float max_norm, float ema_decay,
                        float grad_scale, void* workspace, size_t workspace_bytes, const unsigned char* lr_group4,
                        const float* lr_scales, void* stream);

/* ------------------------------------------------------------------------------------------
 * DEKD logit loss + gradient in one launch.  Replaces DistillLoss.forward (utils/losses.py:156-177)
 * with a timm SoftTargetCrossEntropy base criterion (distill_sub.py:348) and its backward.
 *   kind: 0 none, 1 soft (KL, tau), 2 hard (CE vs argmax of teacher logits, ties -> lowest index)
 *   loss3 = {total, base, distill};  dlogits / dlogits_kd = d total / d logits (upstream grad 1).
 * ---------------------------------------------------------------------------------------- */
DEVIT_API int devit_cls_distill_loss(const float* logits, const float* logits_kd, const float* teacher_logits,
                           const float* soft_targets, int B, int C, int kind, float alpha, float tau, float* loss3,
                           float* dlogits, float* dlogits_kd, void* stream);

/* Token feature-matching loss of the ensemble stage (EnsLoss, utils/losses.py:194,228,241-242: nn.MSELoss):
 * loss[0] (+)= mean((a - b)^2); da (optional) = 2 (a - b) / n. */
DEVIT_API int devit_token_mse(const float* a, const float* b, size_t n, float* loss, float* da, int accumulate, void* stream);

/* EnsLoss loss_type='kldiv' (utils/losses.py:192-193,228,241-242):
 * nn.KLDivLoss(reduction="batchmean", log_target=True)(input = student tokens s, target = teacher tokens t),
 * both taken as log-probabilities as they stand (nothing is normalised or clamped):
 *   loss[0] (+)= sum_i exp(t_i) * (t_i - s_i) / batch;    ds (optional) = -exp(t_i) / batch
 * n = batch * token width.  DEVIT_ERR_ARG for a null s / t / loss or n == 0, DEVIT_ERR_SHAPE for batch <= 0 or
 * n % batch != 0; nothing is launched then.  Deterministic (fixed summation order), no allocation, no sync. */
DEVIT_API int devit_token_kldiv(const float* s, const float* t, size_t n, int batch, float* loss, float* ds,
                                int accumulate, void* stream);

/* ------------------------------------------------------------------------------------------
 * q/k/v feature-relation loss (utils/losses.py:307-328).  The per-image Grams F F^T run on
 * devit_gemm_bf16 (batched, padded to 256x256, DEVIT_EPI_STORE_F32); these two kernels do the rest:
 * stats: row log-sum-exp of gram / sqrt(head_dim) for teacher and student, per-row KL, and
 *        loss = sum_{b,i,j} e^{t}(t - s) / B   (KLDivLoss batchmean, log_target)
 * grad : S = G + G^T, G = (softmax_s - softmax_t) * upstream / (B sqrt(hd_s)), bf16 [B][256][256],
 *        zero outside N x N; then dF_student = S F_student on devit_gemm_bf16.
 * ---------------------------------------------------------------------------------------- */
DEVIT_API int devit_relation_stats(const float* gram_t, const float* gram_s, int B, int N, int ldr, int head_dim_t,
                         int head_dim_s, float* lse_t, float* lse_s, float* row_kl, float* loss, void* stream);
DEVIT_API int devit_relation_grad(const float* gram_t, const float* gram_s, const float* lse_t, const float* lse_s,
                        const float* upstream, int B, int N, int ldr, int head_dim_t, int head_dim_s, void* S_out,
                        int out_is_f32, void* stream);
/* The same loss with both Grams kept on chip (csrc/relation.hip): two launches for all three components, no fp32 Gram in memory.
 * The packed 16-bit qkv buffers are read in place: component j in columns [j D, (j + 1) D), image b in rows [b N, (b + 1) N), row strides
 * ld_s / ld_t elements.  Rows >= N of an image's window are never read.  N <= 208, Ds and Dt multiples of 64 up to 1024, ld multiples of 8
 * and >= 3 D (DEVIT_ERR_SHAPE otherwise); teacher_f16: the teacher buffer holds IEEE f16 instead of bf16.
 *   fwd : lse_t, lse_s, row_kl: fp32 [3][B N] (row log-sum-exps of gram / sqrt(head_dim) and the rows' KL terms, as devit_relation_stats);
 *         loss3[j] = sum(row_kl[j]) / B in a fixed order;
 *         S_out: bf16 [3][B][208][224], every element written:
 *             S_unit = (softmax_s + softmax_s^T - softmax_t - softmax_t^T) / (B sqrt(hd_s)), rounded once, zero outside N x N
 *   bwd : d[b N + i][j Ds + c] = bf16(upstream3[j] * sum_k S_unit[j][b][i][k] F_s[b N + k][j Ds + c]): fp32 sum, the device scalar applied in
 *         fp32, one rounding.  Rows >= B N of d and columns >= 3 Ds are not touched; rows < B N are all written.
 * No atomics: both give the same bits on every run. */
DEVIT_API int devit_relation_fused_fwd(const void* s_qkv, const void* t_qkv, int B, int N, int Ds, int Dt, int ld_s, int ld_t,
                             int head_dim_t, int head_dim_s, int teacher_f16, float* lse_t, float* lse_s, float* row_kl,
                             void* S_out, float* loss3, void* stream);
DEVIT_API int devit_relation_fused_bwd(const void* S, const void* s_qkv, const float* upstream3, int B, int N, int Ds, int ld_s, void* d,
                             int ld_d, void* stream);

/* ------------------------------------------------------------------------------------------
 * cal_qkv_loss / cal_qkv_loss2 / soft_cross_entropy (utils/losses.py:37-41, 247-292; csrc/qkvce.hip).
 *
 * One (student, teacher) layer pair of packed 16-bit qkv buffers, read in place as devit_relation_fused_fwd reads them.  X_i: the [N][D] rows of
 * component i of an image under `layout`: 0 ("view") the reference's `.contiguous().view(B, N, H * 64)` of [B, H, N, 64], a reinterpretation --
 * chunk m of row r is head (r H + m) / N, token (r H + m) % N, each model with its own H = D / 64; 1 ("tokens") head-concatenated token rows.
 * Z_ij = X_i X_j^T / 8 for student and teacher; an ordered pair's term is mean over the B N rows of -sum_j softmax(Z_t)_rj log_softmax(Z_s)_rj.
 * cross 0: the three pairs (i, i), P = 3; cross 1: all nine ordered pairs, P = 9 (six Grams: (j, i) is (i, j) with the softmax over columns).
 *   fwd : terms: fp32 [P][B N] workspace, the rows' terms of ordered pair (i, j) in slot i (cross 0) or 3 i + j (cross 1);
 *         loss[0] = sum(terms) / (P layers B N) in a fixed order;
 *         S_out: bf16 [P][B][208][224], every element written: slot (i, j) holds
 *             S_ij = (dP_rows(Z_ij) + dP_cols(Z_ij)) / (P layers B N 8),  dP = softmax(Z_s) - softmax(Z_t),
 *         rounded once, zero outside N x N; slot (j, i) its transpose.
 *   bwd : d_i = bf16(upstream[0] * sum_j S_ij X_j) (cross 0: j = i alone), fp32 sum, the device scalar applied in fp32, one rounding; the 64-wide
 *         chunks are stored through the layout's map, one writer each.  Rows < B N of the three component column blocks of d are all written;
 *         rows >= B N and columns >= 3 Ds are not touched.
 * N <= 208, Ds and Dt multiples of 64 up to 1024, head_dim 64 for both models, ld multiples of 8 (ld_d: of 4) and >= 3 D: DEVIT_ERR_SHAPE otherwise.
 * cross / layout outside {0, 1}, layers <= 0, a null or misaligned (16 bytes; d: 8) pointer: DEVIT_ERR_ARG.  Nothing is launched on a refusal.
 *
 * soft_cross_entropy on fp32 rows [R][C], R, C >= 1 (DEVIT_ERR_SHAPE otherwise):
 *   fwd : row_loss: fp32 [R] workspace; loss[0] = mean over the rows of -sum_j softmax(targets)_j log_softmax(predicts)_j
 *   bwd : d_predicts = (softmax(predicts) - softmax(targets)) upstream[0] / R
 * No atomics: all four give the same bits on every run.
 * ---------------------------------------------------------------------------------------- */
DEVIT_API int devit_qkv_pair_fwd(const void* s_qkv, const void* t_qkv, int B, int N, int Ds, int Dt, int ld_s, int ld_t, int head_dim_s,
                       int head_dim_t, int teacher_f16, int cross, int layout, int layers, float* terms, void* S_out, float* loss,
                       void* stream);
DEVIT_API int devit_qkv_pair_bwd(const void* S, const void* s_qkv, const float* upstream, int B, int N, int Ds, int ld_s, int head_dim_s,
                       int cross, int layout, void* d, int ld_d, void* stream);
DEVIT_API int devit_soft_ce_rows_fwd(const float* predicts, const float* targets, int R, int C, float* row_loss, float* loss, void* stream);
DEVIT_API int devit_soft_ce_rows_bwd(const float* predicts, const float* targets, const float* upstream, int R, int C, float* d_predicts,
                           void* stream);

/* ------------------------------------------------------------------------------------------
 * Hidden-state distillation (csrc/hid.hip).
 *
 * devit_add_scale_cast_bf16: a gradient that arrives for an exposed encoder output, injected between two devit_block_bwd calls:
 *   dx[m][d] += add[m][d] (fp32, in place);  g_bf16[m][d] = bf16((dx + add)[m][d] * (rowscale ? rowscale[m / rows_per_scale] : 1))
 * -- the fp32 add is torch's, the bf16 value one rounding of the scaled sum, as devit_scale_cast_bf16's.  Rows >= M are not touched.
 *
 * cal_hid_relation_loss (utils/losses.py:295-304) for one (student, teacher) pair of fp32 [B][N][D] hidden states:
 *   loss = mean_{b,i,j} (G_s - G_t)^2 / layers,  G = h^ h^T per image,  h^ = h / max(|h|, eps)
 * The Grams and dh^ = S h^ run on the batched devit_gemm_bf16 (256 x 256 windows per image, as the q/k/v relation loss) or, in exact
 * mode, on devit_gemm_f32; these four entry points do the rest.  N <= 208, D a multiple of 64 up to 1024 (DEVIT_ERR_SHAPE otherwise).
 *   normalize     : out[rows_total][ld] = h^ as bf16 (out_is_f32: fp32), ld a multiple of 128 >= D; columns >= D and rows >= B N are
 *                   written as zeros; inv[B N] = 1 / max(|h|, eps)
 *   stats         : row_sq[B N] (workspace) and loss[0] = sum (G_s - G_t)^2 / (B N^2 layers) over the padded fp32 Grams [B][256][256];
 *                   fixed summation order
 *   grad          : S = (4 upstream / (B N^2 layers)) (G_s - G_t), bf16 (out_is_f32: fp32) [B][256][256], zero outside N x N;
 *                   upstream: device scalar or NULL (= 1)
 *   normalize_bwd : dh[B N][D] = inv (dh^ - h^ (h^ . dh^)) in fp32; hn as normalize wrote it, dhn fp32 with the same leading dimension
 * ---------------------------------------------------------------------------------------- */
DEVIT_API int devit_add_scale_cast_bf16(float* dx, const float* add, void* g_bf16, const float* rowscale, int rows_per_scale, int M,
                              int D, void* stream);
DEVIT_API int devit_hid_normalize(const float* h, void* out, float* inv, int B, int N, int D, int ld, int rows_total, int out_is_f32,
                        float eps, void* stream);
DEVIT_API int devit_hid_stats(const float* gram_s, const float* gram_t, int B, int N, int ldr, int layers, float* row_sq, float* loss,
                    void* stream);
DEVIT_API int devit_hid_grad(const float* gram_s, const float* gram_t, const float* upstream, int B, int N, int ldr, int layers,
                   void* S_out, int out_is_f32, void* stream);
DEVIT_API int devit_hid_normalize_bwd(const void* hn, const float* dhn, const float* inv, float* dh, int B, int N, int D, int ld,
                            int hn_is_f32, void* stream);

/* ------------------------------------------------------------------------------------------
 * Exact-fp32 companion path ("parity mode", csrc/sgemm.hip): the same op sequences with fp32 activations and
 * k-ordered fmaf accumulation, for asserting BASELINE.json's 1e-3 logit bar against the reference's fp32 CPU
 * path.  Not tuned (a few TFLOP/s); never used by bench.py.
 *   devit_gemm_f32: C[z][m][n] = alpha * (batch_scale ? batch_scale[z % batch_inner] : 1) *
 *                                sum_k A[z][m*sam + pk(k)*sak] * B[z][n*sbn + k*sbk]  (+ epilogue, fp32 flavours of
 *     STORE_F32 / GELU / DGELU / RESIDUAL / PATCH; accumulate != 0 adds into out for STORE_F32)
 *     batch z = zo * batch_inner + zi uses ptr + zo * bs_outer + zi * bs_inner (image / head);
 *     pk(k) = k_group > 0 ? k + k_skip * (k / k_group + 1) : k   (A only; patch-embed wgrad)
 *   devit_softmax_rows_f32 / devit_softmax_bwd_rows_f32: in-place row softmax of scale*S (+ natural-log LSE) and
 *     its backward dS = scale * P * (dP - sum_j P dP): with the GEMM above they restate de_vit.py:70-74.
 * ---------------------------------------------------------------------------------------- */
DEVIT_API int devit_gemm_f32(const float* A, long long sam, long long sak, long long a_bs_outer, long long a_bs_inner,
                   const float* B, long long sbn, long long sbk, long long b_bs_outer, long long b_bs_inner, int M, int N,
                   int K, int batch, int batch_inner, long long c_bs_outer, long long c_bs_inner, int k_group, int k_skip,
                   float alpha, const float* batch_scale, int accumulate, const devit_epilogue* ep, void* stream);
DEVIT_API int devit_softmax_rows_f32(float* S, int rows, int ncols, int ld, float scale, float* lse, void* stream);
DEVIT_API int devit_softmax_bwd_rows_f32(const float* P, float* dP, int rows, int ncols, int ld, float scale, void* stream);
DEVIT_API int devit_im2row_f32(const float* img, float* rows, int B, void* stream);          /* [B,3,224,224] -> f32 [B*196][768] */
DEVIT_API int devit_im2row_f32_sized(const float* img, float* rows, int B, int H, int W, void* stream);   /* [B,3,H,W] -> [B*T][768] */
DEVIT_API int devit_scale_rows_f32(const float* src, float* dst, const float* rowscale, int rows_per_scale, int M, int D,
                         void* stream);
DEVIT_API int devit_colsum_f32(const float* y, int M, int N, int ld, float* out, int accumulate, void* stream);

/* ------------------------------------------------------------------------------------------
 * Gradient exchange of the data-parallel step (distill_sub.py:333: DistributedDataParallel's reducer):
 * RCCL all-reduce over xGMI, one communicator per process (= per GPU).  RCCL is bound at run time (dlopen; a copy the
 * process already holds, e.g. PyTorch's, is reused), so the library has no link-time dependency on it.
 *   devit_comm_unique_id: rank 0 creates the 128-byte rendezvous id and hands it to the other ranks by any host
 *     channel (the launcher's store, a file, torch.distributed's object broadcast).
 *   devit_comm_init: collective over all ranks; uses the calling thread's current HIP device.
 *   devit_comm_allreduce_f32: in-place SUM of buf[count] on `stream` (asynchronous, like every other entry point);
 *     the caller scales by 1/world (devit_adamw_step's grad_scale) -- one bucket of the flat gradient buffer per call.
 * ---------------------------------------------------------------------------------------- */
#define DEVIT_COMM_ID_BYTES 128
DEVIT_API int devit_comm_unique_id(void* id /* [DEVIT_COMM_ID_BYTES] host */);
DEVIT_API int devit_comm_init(const void* id, int rank, int world, void** comm);
DEVIT_API int devit_comm_allreduce_f32(void* comm, float* buf, size_t count, void* stream);
DEVIT_API int devit_comm_destroy(void* comm);

/* ------------------------------------------------------------------------------------------
 * The encoder blocks with dropout p > 0 (section "Dropout" above): devit_encoder_fwd / devit_block_bwd with one devit_block_dropout per block
 * beside the existing structs.  thr == 0 and thr_attn == 0 launch exactly what the plain entry points launch.  Otherwise, same order of
 * kernels with these differences -- forward: attention through devit_attn_fwd_drop (thr_attn > 0); GELU epilogue, then devit_dropout_apply on
 * the hidden (site 3); proj and fc2 store fp32 into `tmp` (DEVIT_EPI_STORE_F32) and devit_dropout_residual forms x1 / x2 (sites 2, 4; the
 * full-row fc2 launch and DEVIT_BLK_ATT are not taken).  Backward: io->g2 is MASKED IN PLACE first (site 4) and fc2's bias gradient is the
 * masked g2's column sums -- so io->g2_bias_done must be 0, and the block ABOVE a block with thr > 0 passes io->prev_fc2_b_grad = NULL --;
 * dh_pre is masked after the dGELU dgrad (site 3); the LayerNorm backward behind fc1's dgrad runs without its column sums, g1 is masked (site 2)
 * and proj's bias gradient comes from the masked g1; attention through devit_attn_bwd_drop.  Weight-gradient jobs read the masked buffers.
 * Compacted blocks index their compact layout.  bf16 blocks only.
 * ---------------------------------------------------------------------------------------- */
typedef struct {
  unsigned long long seed; /* the forward's seed */
  int block;               /* the block's index in the model: part of every counter */
  unsigned thr, thr_attn;  /* thresholds of drop (sites 2, 3, 4) and attn_drop (site 1); 0 = that dropout is off */
  float scale_keep, scale_keep_attn; /* 1 / (1 - p) */
  float* tmp;              /* fp32 [pad_rows(M)][D] scratch (thr > 0), may be shared by all blocks of a call */
} devit_block_dropout;
DEVIT_API int devit_encoder_fwd_drop(int nblocks, const devit_block_weights* w, const devit_block_acts* acts, const devit_block_dropout* drop,
                           int B, int N, int D, float eps, void* stream);
DEVIT_API int devit_block_bwd_drop(const devit_block_weights* w, const devit_block_acts* acts, const devit_block_wgrads* grads,
                         const devit_block_bwd_io* io, const devit_block_dropout* drop, int B, int N, int D, float eps, void* stream);

/* ------------------------------------------------------------------------------------------
 * Input augmentation: a resident uint8 image set -> the normalized fp32 batch [B,3,S,S] that Mixup and the patch-row kernels consume.
 * It replaces, per sample, timm's transforms_imagenet_train as data/get_dataset.py:71-97 configures it (RandomResizedCrop / RandomCrop with
 * padding, horizontal flip, ToTensor, Normalize, RandomErasing) and the eval stack (Resize, CenterCrop, ToTensor, Normalize); every random
 * draw is the host's and arrives in a device table of B devit_augment_sample (struct id 14 of devit_abi_struct_size, 120 bytes).
 *   src    uint8 [n][H0][W0][3] (HWC), idx int32 [B] on the device: out[b] is made from image idx[b] (clamped to 0 .. n-1)
 *   out    fp32 [B][3][S][S], S one of the patch-cutting kernels' sizes (a multiple of 16 from 32 to 224), 16-byte aligned
 * Per output pixel (y, x) of sample b, in this order:
 *  1 crop, then resize -- PIL's Image.crop((x0, y0, x0 + w, y0 + h)).resize((Rw, Rh), filter) on the uint8 values, of which the
 *    window [oy, oy + S) x [ox, ox + S) is produced (train: Rh = Rw = S, oy = ox = 0; eval: the resized side with a centred window).
 *    Per axis, with len the box side and R the virtual side: scale = len / R, fs = max(scale, 1), support = (1 bilinear | 2 bicubic) * fs;
 *    for the virtual index xx: center = (xx + 0.5) * scale, xmin = max(int(center - support + 0.5), 0), xmax = min(int(center + support
 *    + 0.5), len); tap k (0 <= k < xmax - xmin) weighs f((k + xmin - center + 0.5) * (1 / fs)), f the triangle or the Keys cubic with
 *    a = -0.5 ( ((a+2)|t| - (a+3)) t^2 + 1 below 1, (((|t| - 5)|t| + 8)|t| - 4) a below 2 ); the weights are divided by their sequential
 *    sum and become integers int(w * 2^22 +- 0.5) (half away from zero).  All of this in IEEE double, uncontracted, in this operation
 *    order (devit_augment_coeffs, a kernel of its own; it is PIL's precompute_coeffs + normalize_coeffs_8bpc).  The horizontal pass runs
 *    first; each pass is clamp((2^21 + sum pixel * weight) >> 22, 0, 255) in int32, and the uint8 between the passes is part of the
 *    definition.  Taps never leave the box.  At most DEVIT_AUGMENT_TAPS taps per axis: a caller refuses sets that would need more.
 *    filter 0 (unit scale): the pixel (y0 + oy + y, x0 + ox + x) itself; the box may then lie partly outside the image (RandomCrop's padding).
 *    A pixel outside the image reads 0 in every mode.
 *  2 horizontal flip of the window (flip != 0): output x takes window column S - 1 - x.
 *  3 ToTensor and Normalize in fp32: v = ((float)u8 / 255.0f - mean[c]) / std[c]  (two correctly rounded divisions, one subtraction).
 *  4 RandomErasing, after Normalize as in timm: inside any of the first n_erase boxes (top, left, h, w) of the OUTPUT the value becomes
 *      erase_mode 0 const: 0;  1 rand: one normal per box and channel;  2 pixel: one normal per channel and pixel
 *    (boxes later in the list win where they overlap; in mode 2 a pixel's normal does not depend on the box).
 *    Normals: Philox4x32-10 as in section "Dropout", key = (seed & 0xffffffff, seed >> 32), counter = (N & 0xffffffff, N >> 32,
 *    DEVIT_AUGMENT_SITE + c, g) with N = noise_base + b and c the channel; mode 2: g = (y * S + x) >> 2 and the pixel takes normal
 *    (y * S + x) & 3 of the call; mode 1: g = 0x80000000 + box index, normal 0.  The four normals of a call's words w0 .. w3 are
 *      z0 = r(w0) cos(2 pi u(w1)), z1 = r(w0) sin(2 pi u(w1)), z2 = r(w2) cos(2 pi u(w3)), z3 = r(w2) sin(2 pi u(w3)),
 *      u(w) = ((w >> 8) + 0.5) * 2^-24, r(w) = sqrt(-2 ln u(w))   (Box-Muller)
 *    evaluated in fp32.  u(w) is exact in fp32 for w >> 8 < 2^23; above, 1 - u(w) is (it is u of the complemented word), and the kernel
 *    goes through it: ln u = log1p(-(1 - u)), cos(2 pi u) = cos(2 pi (1 - u)), sin(2 pi u) = -sin(2 pi (1 - u)).  So the inputs of the
 *    four library functions (logf / log1pf, sqrtf, sincospif) carry no rounding error of their own.
 * devit_augment_workspace(B, S): bytes of the coefficient workspace (int32 [B][2 axes][2 + DEVIT_AUGMENT_TAPS][S]: xmin, count, weights).
 * devit_augment_coeffs fills it from the table; devit_augment_batch runs devit_augment_coeffs and then the resampling kernel, which is
 * integer arithmetic up to step 3.  mean / std are HOST arrays of 3 floats.  No address in either kernel depends on the table's or idx's contents
 * without a clamp, so both are memory-safe for any table bytes; rows of `out` beyond B and bytes outside `out` are never written.
 * Sets whose images differ in size, and samples that need more than DEVIT_AUGMENT_TAPS taps: "Packed sets" below (devit_augment_ragged).
 * ---------------------------------------------------------------------------------------- */
#define DEVIT_AUGMENT_TAPS 12
#define DEVIT_AUGMENT_MAX_ERASE 4
#define DEVIT_AUGMENT_SITE 0x100u /* word 2 of the noise counter is this + channel: no dropout site (0 .. 4) shares a counter with it */
enum devit_augment_filter { DEVIT_AUG_NONE = 0, DEVIT_AUG_BILINEAR = 1, DEVIT_AUG_BICUBIC = 2 };
enum devit_augment_erase { DEVIT_AUG_ERASE_CONST = 0, DEVIT_AUG_ERASE_RAND = 1, DEVIT_AUG_ERASE_PIXEL = 2 };
typedef struct {
  int y0, x0, h, w;     /* source box; y0 / x0 may be negative with filter 0 */
  int Rh, Rw, oy, ox;   /* virtual output size and the window's offset in it */
  int filter;           /* devit_augment_filter */
  int flip;
  int n_erase;          /* 0 .. DEVIT_AUGMENT_MAX_ERASE */
  int erase_mode;       /* devit_augment_erase */
  int erase[DEVIT_AUGMENT_MAX_ERASE][4]; /* top, left, h, w in the output */
  unsigned long long noise_base;
} devit_augment_sample;
DEVIT_API size_t devit_augment_workspace(int B, int S);
DEVIT_API int devit_augment_coeffs(const devit_augment_sample* table /* device, B entries */, int B, int S, void* workspace,
                         size_t workspace_bytes, void* stream);
DEVIT_API int devit_augment_batch(const unsigned char* src, int n, int H0, int W0, const int* idx, const devit_augment_sample* table, int B,
                        int S, const float* mean /* host [3] */, const float* std /* host [3] */, unsigned long long seed, float* out,
                        void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Image ops: RandAugment's fifteen `rand-...-inc1` operations (timm 0.5.4 auto_augment.py, _RAND_INCREASING_TRANSFORMS) and the three
 * enhancement steps of ColorJitter without hue, on the S x S uint8 window between step 2 (flip) and step 3 (ToTensor) above, bit for bit as
 * PIL computes them.  Every draw is the host's: sample b applies layers 0 .. n_ops - 1 of entry b of a device table of devit_augment_ops
 * (struct id 15 of devit_abi_struct_size, 328 bytes), each layer on the result of the one before.  A layer is (op, filter, factor, arg,
 * matrix, fill); u is a uint8 level of the layer's input, all of the image is read before any of it is replaced.
 *   Invert        255 - u
 *   Posterize     u & ~(2^(8 - arg) - 1), arg = bits clamped to 0 .. 8 (0: black)
 *   Solarize      u if u < arg else 255 - u
 *   SolarizeAdd   min(255, u + arg) if u < 128 else u
 *   AutoContrast  per channel, lo / hi the first / last non-empty bin of its histogram: unchanged if hi <= lo, else scale = 255.0 / (hi - lo),
 *                 off = -lo * scale, u -> clamp(int(u * scale + off), 0, 255) in IEEE double, uncontracted (int truncates toward zero)
 *   Equalize      per channel with histogram h: unchanged with at most one non-empty bin; step = (sum of the bins - the last non-empty
 *                 bin) / 255 in integers, unchanged if 0; else u -> min(255, (step / 2 + sum of h[0 .. u-1]) / step) in integers
 *   blend(d, u, f) = d + f * (u - d) in fp32: operands converted to float, f rounded to float, one multiply and one add, NOT fused;
 *                 truncated toward zero for 0 <= f <= 1, else 0 if <= 0, 255 if >= 255, else truncated
 *   Brightness    blend(0, u, factor)
 *   Color         blend(L, u, factor), L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16 of the pixel, for all three channels
 *   Contrast      blend(m, u, factor), m = int(sum of L over the image / (S * S) + 0.5): integer sum, one double division
 *   Sharpness     blend(s, u, factor), s = PIL's ImageFilter.SMOOTH: the one-pixel border is the image's; inside, a fp32 accumulation from 0,
 *                 row-major over the 3 x 3 window, of pixel * (k / 13.0f) with k = 1 except 5 at the centre (each product rounded, then each
 *                 sum), then + 0.5f; 0 if <= 0, 255 if >= 255, else truncated
 *   Rotate, ShearX, ShearY, TranslateX, TranslateY   Image.transform(AFFINE, matrix, filter, fillcolor = fill): the matrix (a, b, c, d, e, f)
 *                 is the host's (ShearX (1, v, 0, 0, 1, 0); ShearY (1, 0, 0, v, 1, 0); TranslateX (1, 0, px, 0, 1, 0); TranslateY (1, 0, 0, 0,
 *                 1, px); Rotate as Image.rotate(deg): t = -radians(deg % 360), a = e = round(cos t, 15), b = round(sin t, 15), d = round(-sin t,
 *                 15), c = a * (-S/2) + b * (-S/2) + S/2, f = d * (-S/2) + e * (-S/2) + S/2); the five op ids run the same code.
 *                 Output pixel (xo, yo), in IEEE double, uncontracted: xin = a (xo + 0.5) + b (yo + 0.5) + c, yin = d (xo + 0.5) + e (yo +
 *                 0.5) + f.  Unless 0 <= xin < S and 0 <= yin < S (a NaN is not) the pixel is the fill colour.  Else xin -= 0.5, x = floor(xin),
 *                 dx = xin - x, the same for y; cl() clamps an index to 0 .. S - 1.
 *                 bilinear: row(r) = p0 + (p1 - p0) * dx on columns cl(x), cl(x + 1) of row r; v1 = row(cl(y)); v2 = row(y + 1) if that row is
 *                 in the image, else v1; result v1 + (v2 - v1) * dy, truncated.
 *                 bicubic: cub(v1, v2, v3, v4, t) = p1 + t (p2 + t (p3 + t p4)), p1 = v2, p2 = -v1 + v3, p3 = 2 (v1 - v2) + v3 - v4,
 *                 p4 = -v1 + v2 - v3 + v4; row(r) = cub over columns cl(x - 1) .. cl(x + 2) at dx; the four row values are row(cl(y - 1)),
 *                 then row(y), row(y + 1), row(y + 2), each replaced by the value before it when its row is outside the image; result
 *                 cub of them at dy: 0 if <= 0, 255 if >= 255, else truncated.
 * Op ids outside 0 .. 14 leave the image as it is; n_ops is clamped to 0 .. DEVIT_AUGMENT_MAX_OPS; a filter other than bicubic is bilinear.
 * The kernel (one workgroup per sample) holds the sample's whole image in LDS -- 150 528 bytes at S = 224 -- through every layer: the
 * histograms and the luminance sum are integer LDS reductions (order-free: the result is deterministic), the pointwise ops run in place
 * through a 3 x 256 table, Sharpness and the affine family compute every output pixel into registers before any is written back.
 *   devit_image_ops          uint8 [B][S][S][3] -> uint8 [B][S][S][3] (in == out is allowed): the layers alone
 *   devit_augment_batch_ops  devit_augment_batch with the layers between steps 2 and 3: steps 1 and 2 leave the uint8 window in the
 *                            workspace, the op kernel loads it, applies the layers and does steps 3 and 4.  With n_ops == 0 for every
 *                            sample its output has the bits of devit_augment_batch's.  devit_augment_ops_workspace(B, S) bytes of workspace
 *                            (the coefficient workspace and the windows behind it).
 * Both are memory-safe for any table bytes: ids, counts and every LDS address are clamped, a non-finite or huge matrix gives fill colour.
 * ---------------------------------------------------------------------------------------- */
#define DEVIT_AUGMENT_MAX_OPS 4
enum devit_image_op {
  DEVIT_OP_AUTOCONTRAST = 0, DEVIT_OP_EQUALIZE = 1, DEVIT_OP_INVERT = 2, DEVIT_OP_ROTATE = 3, DEVIT_OP_POSTERIZE = 4, DEVIT_OP_SOLARIZE = 5,
  DEVIT_OP_SOLARIZE_ADD = 6, DEVIT_OP_COLOR = 7, DEVIT_OP_CONTRAST = 8, DEVIT_OP_BRIGHTNESS = 9, DEVIT_OP_SHARPNESS = 10,
  DEVIT_OP_SHEAR_X = 11, DEVIT_OP_SHEAR_Y = 12, DEVIT_OP_TRANSLATE_X = 13, DEVIT_OP_TRANSLATE_Y = 14, DEVIT_OP_COUNT = 15
};
typedef struct {
  int n_ops;                              /* 0 .. DEVIT_AUGMENT_MAX_OPS */
  int reserved;
  int op[DEVIT_AUGMENT_MAX_OPS];          /* devit_image_op */
  int filter[DEVIT_AUGMENT_MAX_OPS];      /* devit_augment_filter of the affine family */
  float factor[DEVIT_AUGMENT_MAX_OPS];    /* the blend ops */
  int arg[DEVIT_AUGMENT_MAX_OPS];         /* Posterize: bits, Solarize: threshold, SolarizeAdd: addend */
  int fill[DEVIT_AUGMENT_MAX_OPS][4];     /* r, g, b of the affine family's fill colour, one spare */
  double matrix[DEVIT_AUGMENT_MAX_OPS][6];
} devit_augment_ops;
DEVIT_API int devit_image_ops(const unsigned char* in, const devit_augment_ops* ops /* device, B entries */, int B, int S, unsigned char* out,
                    void* stream);
DEVIT_API size_t devit_augment_ops_workspace(int B, int S);
DEVIT_API int devit_augment_batch_ops(const unsigned char* src, int n, int H0, int W0, const int* idx, const devit_augment_sample* table,
                            const devit_augment_ops* ops, int B, int S, const float* mean /* host [3] */, const float* std /* host [3] */,
                            unsigned long long seed, float* out, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Packed sets: the "Input augmentation" stage over a set whose images differ in size.  The set is one byte arena on the device, the
 * images HWC one behind the other, and a device directory of n devit_image_entry (struct id 16 of devit_abi_struct_size, 16 bytes): the image's byte offset in
 * the arena (a multiple of 16 as devit_amd.data packs it; the kernels need no alignment) and its H and W.  out[b] is made from image
 * clamp(idx[b], 0, n - 1) by steps 1 to 4 of that section, unchanged, with H0 and W0 that entry's; with ops != null the layers of "Image ops" above
 * run between steps 2 and 3 as in devit_augment_batch_ops (with n_ops == 0 everywhere: the same bits as with ops == null).
 *   max_taps  the caller's upper bound T, 1 .. DEVIT_AUGMENT_TAPS_MAX, on the taps any sample of the batch needs on either axis.
 *             The coefficient workspace is int32 [B][2 axes][2 + T][S] (xmin, count, weights; counts are clamped to T);
 *             devit_augment_ragged_workspace(B, S, max_taps, with_ops) bytes, with_ops != 0 adding the uint8 windows behind it.
 *   A sample is WIDE when bound(h, Rh) or bound(w, Rw) exceeds DEVIT_AUGMENT_TAPS, with, in IEEE double,
 *             bound(len, R) = min(floor(2 * support) + 1, len), support = (1 bilinear | 2 bicubic) * max(len / R, 1); filter 0: 1.
 *             The bound is never below the exact tap count of the axis (and at most 1 above it), so a sample that is not wide fits the
 *             narrow kernel.  max_taps is at least the largest bound of the batch's samples (or the exact count where the caller knows it).
 * Two resampling kernels serve a batch, each launched over all B when max_taps > DEVIT_AUGMENT_TAPS; a workgroup leaves at once unless its
 * sample is its kernel's kind, decided from the table row by the closed form above (no host decision per sample, no divergence in a wave).
 *   narrow    devit_augment_batch's kernel with the image's base, H0 and W0 read from the directory: 12 weights in registers per column, the
 *             uint8 intermediate of up to 24 source rows in LDS.
 *   wide      13 .. DEVIT_AUGMENT_TAPS_MAX taps.  One workgroup per (sample, 16 output rows), thread x owning output column x: it walks the
 *             band's source rows once, makes each row's horizontal result for its column (weights read [tap][x] from the workspace), clamps
 *             it to uint8 -- PIL's intermediate, part of the definition -- and adds it, weighted, into the int32 accumulators of the output
 *             rows whose vertical window holds that source row.  No intermediate image is kept, so a band may span any number of rows.
 * Both compute the same integers: a sample gives identical bits through either (DEVIT_AUGMENT_FORCE_WIDE in flags sends every sample
 * through the wide kernel; tests compare).  The pass order is horizontal first for every box (PIL itself makes the vertical pass first for
 * boxes about 107 or more times as tall as wide).
 * Memory safety: idx is clamped; every source address is clamped into the image's own extent, which is checked against [0, arena_bytes)
 * per sample, and the value masked afterwards; an entry with H < 1, W < 1 or offset + 3 H W > arena_bytes reads as an image of zeros;
 * counts and every LDS index are clamped; rows of `out` beyond B and bytes outside `out` are never written.
 * ---------------------------------------------------------------------------------------- */
#define DEVIT_AUGMENT_TAPS_MAX 128
#define DEVIT_AUGMENT_FORCE_WIDE 1u /* flags: every sample through the wide kernel (tests) */
typedef struct {
  unsigned long long offset; /* of the image's first byte in the arena */
  int H, W;
} devit_image_entry;
DEVIT_API size_t devit_augment_ragged_workspace(int B, int S, int max_taps, int with_ops);
DEVIT_API int devit_augment_ragged(const unsigned char* arena, size_t arena_bytes, const devit_image_entry* entries /* device, n */, int n,
                         const int* idx, const devit_augment_sample* table, const devit_augment_ops* ops /* may be null */, int B,
                         int S, const float* mean /* host [3] */, const float* std /* host [3] */, unsigned long long seed, float* out,
                         void* workspace, size_t workspace_bytes, int max_taps, unsigned flags, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DEVIT_HIP_H */
