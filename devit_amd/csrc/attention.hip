// Fused multi-head attention forward / backward for ViT token counts (N <= 208, head_dim = 64).
// One workgroup (4 waves) per (image, head): the whole head's K and V live in LDS, the N x N
// score matrix never reaches HBM.  Replaces models/de_vit.py:68-79 (q k^T * scale -> softmax ->
// @ v -> transpose -> head gate) and its autograd backward.
//
// qkv layout = output of the qkv GEMM: row (b, n), feature j*D + h*64 + e (j = q,k,v)
// (models/de_vit.py:67 reshape(B,N,3,H,hd)); out layout [B*N][D] with feature h*64 + e (:74,:81).
//
// LDS images are [rows][64] bf16 (128-byte rows); 16-byte chunk c of row r is stored at chunk
// c ^ ((r >> 1) & 7): conflict-free ds_read_b128 row fragments, 2-way ds_read_b64_tr_b16.
#include <stdlib.h>

#include "devit_common.h"
#include "dropout.h"

namespace {

constexpr int HD = 64;            // head dim
constexpr int MAXT = 13;          // 16-row tiles: N <= 208
constexpr int KROWS = 224;        // 7 k-steps of 32
constexpr int PSTRIDE = 232;      // bf16 elements per P / dS row (464 B, 16-B multiple)
constexpr int IMG_BYTES = KROWS * HD * 2;  // 28672

__device__ __forceinline__ int img_off(int row, int chunk) { return row * 128 + ((chunk ^ ((row >> 1) & 7)) << 4); }

// MFMA fragment with 8 consecutive d (k = d) for rows r0 + (lane & 15): A of Q K^T, B = K rows, ...
__device__ __forceinline__ bf16x8 img_row_frag(const char* img, int r0, int kk, int lane) {
  return *(const bf16x8*)(img + img_off(r0 + (lane & 15), kk * 4 + (lane >> 4)));
}
// MFMA fragment whose k index is the image ROW (k0..k0+31) and whose row/col index is d (c0..c0+15).
__device__ __forceinline__ bf16x8 img_tr_frag(const char* img, int k0, int c0, int lane) {
  const int G = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
  const int r = k0 + G * 8 + q, ch = (c0 >> 3) + (p >> 1), sub = (p & 1) * 8;
  return cat8(lds_tr_read(img + img_off(r, ch) + sub), lds_tr_read(img + img_off(r + 4, ch) + sub));
}
// P / dS buffers: [rows][PSTRIDE] bf16, unswizzled.
__device__ __forceinline__ bf16x8 pbuf_row_frag(const char* buf, int r0, int ks, int lane) {
  return *(const bf16x8*)(buf + (r0 + (lane & 15)) * (PSTRIDE * 2) + (ks * 32 + (lane >> 4) * 8) * 2);
}
__device__ __forceinline__ bf16x8 pbuf_tr_frag(const char* buf, int k0, int c0, int lane) {
  const int G = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
  const char* a = buf + (k0 + G * 8 + q) * (PSTRIDE * 2) + (c0 + p * 4) * 2;
  return cat8(lds_tr_read(a), lds_tr_read(a + 4 * PSTRIDE * 2));
}

// Rows [0, KROWS) of a strided [N][64] bf16 matrix -> registers -> an LDS image (rows >= N zero).  Only the backward's dO / O
// rows still travel this way (delta needs them in registers); every other image arrives by LDS-DMA, see dma_image().
template <int NT>
struct RowRegs {
  static constexpr int ITERS = (KROWS * 8 + NT - 1) / NT;
  bf16x8 v[ITERS];
};
template <int NT>
__device__ __forceinline__ void fetch_rows(RowRegs<NT>& r, const __bf16* src, size_t row_stride, int N, int tid) {
#pragma unroll
  for (int it = 0; it < RowRegs<NT>::ITERS; ++it) {
    const int idx = tid + it * NT, row = idx >> 3, c = idx & 7;
    // unconditional load from a clamped row, zeroed afterwards: a load under a per-element condition makes hipcc branch
    // around it and wait for each one in turn (one HBM round trip per iteration)
    r.v[it] = *(const bf16x8*)(src + (size_t)min(row, N - 1) * row_stride + c * 8);
  }
#pragma unroll
  for (int it = 0; it < RowRegs<NT>::ITERS; ++it) {
    const bf16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
    if ((tid + it * NT) >> 3 >= N) r.v[it] = z;
  }
}
template <int NT>
__device__ __forceinline__ void put_image(char* img, const RowRegs<NT>& r, float mul, int tid) {
#pragma unroll
  for (int it = 0; it < RowRegs<NT>::ITERS; ++it) {
    const int idx = tid + it * NT, row = idx >> 3, c = idx & 7;
    bf16x8 v = r.v[it];
    if (mul != 1.0f) {
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = f2bf(bf2f(v[e]) * mul);
    }
    if (row < KROWS) *(bf16x8*)(img + img_off(row, c)) = v;
  }
}

// Rows [0, KROWS) of a strided [N][64] 16-bit matrix -> an LDS image by LDS-DMA: one wave-instruction moves 8 rows x 128 B
// (1 KiB) into consecutive LDS bytes, so the image's chunk swizzle goes on the per-lane SOURCE address (lane l of slab s
// writes row 8 s + l / 8, physical chunk l % 8, which must hold logical chunk (l % 8) ^ swizzle(row)).  Rows >= N cannot
// be zero-filled by a DMA: they repeat row N - 1 (finite values; every use of a padded key or query is masked to P = 0).
template <int NWAVES, int ROWS = KROWS>
__device__ __forceinline__ void dma_image(char* img, const __bf16* src, size_t row_stride, int N, int wave, int lane) {
#pragma unroll
  for (int it = 0; it < (ROWS / 8 + NWAVES - 1) / NWAVES; ++it) {
    const int slab = wave + it * NWAVES;
    if (slab < ROWS / 8) {
      const int row = slab * 8 + (lane >> 3), c = (lane & 7) ^ ((row >> 1) & 7);
      const __bf16* g = src + (size_t)min(row, N - 1) * row_stride + c * 8;
      // (default cache policy: a non-temporal DMA is 18 % faster from cold HBM -- 51 / 92 against 62 / 113 us forward -- and
      // no faster in the step, where much of qkv is still in the Infinity Cache: profiles/r03_t_attention_nt_loads.txt)
      __builtin_amdgcn_global_load_lds(GLB_PTR(g), LDS_PTR(img + slab * 1024), 16, 0, 0);
    }
  }
}

// Query side and key side are described separately: the packed form (devit_attn_fwd) points all three at one qkv buffer
// with NQ == N; the rows form (devit_attn_fwd_rows) reads NQ <= N query rows per image from a buffer of their own -- the
// last block of a model whose caller consumes only the class / distillation tokens (models/de_vit.py:286-288).
struct AttnFwdArgs {
  const __bf16* q;      // [B*NQ][q_rs], feature h*64 + e
  const __bf16* k;      // [B*N][kv_rs]
  const __bf16* v;
  __bf16* out;          // [B*NQ][H*64]
  float* lse;           // [B][H][NQ]
  const float* head_gate;
  int B, N, NQ, H;
  int q_rs, kv_rs;
  float scale;
};

// Forward.  S^T = K Q^T puts the QUERY on the MFMA lane (col = lane & 15) and the keys in the accumulator
// registers, so the row softmax is in-lane + two shuffles, and the bf16 P values of two key tiles are already
// the B operand of O^T = V^T P (k-slot (g, j) = key 16*t(j>>2) + 4g + (j&3); V is read transposed with the
// same key order).  P never touches LDS; each lane ends up with 4 consecutive d of its own query row.
// -DDEVIT_ATTN_FWD_WAVES=4 (round-3 experiment, measured null): 4 waves, images of 208 rows (13 key tiles), 53 KB per
// workgroup -> THREE workgroups per CU instead of two.  Half of a workgroup's life is its prologue (in-kernel stamps,
// tools/attn_fwd_stamps.py), but a third resident workgroup only makes every prologue longer: 62.6 / 110 us against
// 62.0 / 111 us per student / teacher launch (profiles/r03_s_attention_fwd_occupancy_null.txt).  The launch runs at the rate
// the memory system delivers first-touch 128-byte row pieces (2.5-2.8 TB/s), whatever the occupancy.
#ifndef DEVIT_ATTN_FWD_WAVES
#define DEVIT_ATTN_FWD_WAVES 8
#endif
constexpr int FWD_WAVES = DEVIT_ATTN_FWD_WAVES;
#ifndef DEVIT_ATTN_OUT_ROWS
#define DEVIT_ATTN_OUT_ROWS 1        // forward output rows leave as whole 128-byte lines through a per-wave LDS slab (0: 32-byte pieces)
#endif
constexpr int OSLAB_ROW = 144;       // bytes per slab row: 128 + 16 (16 rows of one column land on 8 different bank groups)
constexpr int FWD_ROWS = FWD_WAVES == 8 ? KROWS : MAXT * 16;           // rows of the K / V images
constexpr int FWD_IMG = FWD_ROWS * HD * 2;

// DROP (attn_fwd_drop_kernel; nn.Dropout on the softmax, models/de_vit.py:72): P is normalised, then masked and scaled by 1 / (1 - p) -- here
// the dropped e^{s - max} are zeroed before they become the MFMA operand and the row's 1 / sum carries the scale; sum and lse are of the
// undropped row.  A lane's four score registers of a key tile are four consecutive keys of its query row: one Philox call (dropout.h).
// The kernel body is csrc/attention_fwd.inc, included once per kernel: the preprocessor (ATTN_DROP), not a template flag, takes the dropout lines
// out, so that attn_fwd_kernel is compiled from the very tokens it had before dropout existed (tools/kernel_digest.py: same machine code).
template <bool F16>
__global__ __launch_bounds__(FWD_WAVES * 64, FWD_WAVES == 8 ? 4 : 3) void attn_fwd_kernel(const AttnFwdArgs a) {
#define ATTN_DROP 0
#include "attention_fwd.inc"
#undef ATTN_DROP
}
template <bool F16>
__global__ __launch_bounds__(FWD_WAVES * 64, FWD_WAVES == 8 ? 4 : 3) void attn_fwd_drop_kernel(const AttnFwdArgs a, const DropKey dk) {
#define ATTN_DROP 1
#include "attention_fwd.inc"
#undef ATTN_DROP
}

// ------------------------------------------------------------------------------------------
// Backward.  Recomputes P from the saved log-sum-exp.  S and dP are computed with the KEY on the MFMA lane, so their
// accumulators (two 16-query tiles = one 32-query block) are already the B operands of dV^T += dO^T P and
// dK^T += Q^T dS: P never touches LDS and each wave keeps dK / dV of its own key tiles in registers for the whole kernel
// (no cross-workgroup reduction, no atomics).  Only dS crosses LDS, once per block, stored transposed ([key][q], 8-byte
// writes), for dQ^T = K^T dS^T.
// ------------------------------------------------------------------------------------------
struct AttnBwdArgs {
  const __bf16* q;      // [B*NQ][q_rs]; query side / key side split as in AttnFwdArgs
  const __bf16* k;      // [B*N][kv_rs]
  const __bf16* v;
  const __bf16* out;    // forward output (post gate)  [B*NQ][D]
  const __bf16* dout;   // gradient wrt forward output [B*NQ][D]
  const float* lse;     // [B][H][NQ]
  const float* head_gate;
  const __bf16* dq_add; // optional extra gradients added in (relation loss), laid out like dq / dk / dv
  const __bf16* dk_add;
  const __bf16* dv_add;
  __bf16* dq;           // [B*NQ][dq_rs]
  __bf16* dk;           // [B*N][dkv_rs]
  __bf16* dv;
  int B, N, NQ, H;
  int q_rs, kv_rs, dq_rs, dkv_rs;
  float scale;
};

__device__ __forceinline__ void store_grad4(__bf16* dst, const __bf16* add, f32x4 v) {
  if (add) {
    const bf16x4 e = *(const bf16x4*)add;
    v += (f32x4){bf2f(e[0]), bf2f(e[1]), bf2f(e[2]), bf2f(e[3])};
  }
  const bf16x4 o = {f2bf(v[0]), f2bf(v[1]), f2bf(v[2]), f2bf(v[3])};
  *(bf16x4*)dst = o;
}

// ------------------------------------------------------------------------------------------
// Two workgroups per CU: 4 waves, <= 256 VGPRs, 79 KB of LDS each.  (Rounds 1-2 ran 8 waves with four [224][64] images in
// LDS, 152 KB: one workgroup per CU, so load -> compute -> store ran strictly one after the other on every CU -- 181 us per
// B = 256, H = 6 launch from cold HBM against 160 us for this form, profiles/r03_*_attention_bwd.txt.)  Only the K image
// stays in LDS (the dQ product needs every key's row); V lives in registers as the row fragments of the wave's own key
// tiles; Q and dO arrive one 32-query block at a time through a four-stage LDS ring filled by LDS-DMA up to three blocks
// ahead (counted vmcnt); the block's Q / dO fragments are re-read from LDS per key tile because 128 accumulator + 32
// V-fragment registers leave no room to hold them.  Two such workgroups share a CU and run out of phase: one loads or
// stores while the other computes.  Same MFMA shapes, operand roundings and reduction order over query blocks / key steps
// as the 8-wave kernel had, except that the head gate multiplies dP and dV in fp32 instead of a bf16 copy of dO: identical
// for the 0/1 gates of core/imp_rank.py.
// In-kernel stamps (tools/attn_stamps.py, -DDEVIT_ATTN_STAMP): a workgroup lives ~47 us = prologue 23 (140 KB of first-touch
// loads at the ~3-6 B/cycle its CU's load path gives it beside the other workgroup) + main loop 22 (bound by
// vector-instruction ISSUE, ~600 instructions per wave and block, not by MFMA or memory: halving the instruction count of
// the softmax-gradient arithmetic took it from 26 to 22) + stores 2.
// ------------------------------------------------------------------------------------------
constexpr int B4_WAVES = 4;
constexpr int B4_KT = (MAXT + 1 + B4_WAVES - 1) / B4_WAVES;      // key tiles per wave (4); tile 13 (keys 208..223) is padding
constexpr int DST4_STRIDE = 36;                                   // bf16 per dS^T row: 32 queries + pad (72-B rows)
constexpr int DST4_BYTES = KROWS * DST4_STRIDE * 2;               // 16128
constexpr int QD_STAGE = 2 * 32 * HD * 2;                         // one ring stage: Q block + dO block, 8192 B
constexpr int QD_NST = 4;                                         // ring stages: three blocks (24 KB per workgroup) in flight
constexpr int BWD4_LDS = IMG_BYTES + QD_NST * QD_STAGE + DST4_BYTES + 2 * KROWS * 4;   // 79360

// one LDS-DMA instruction (1 KiB: 8 rows x 128 B) from per-lane global addresses to LDS byte address `lds`; inline asm so
// that hipcc's waitcnt pass does not put a vmcnt(0) in front of every later ds_read (gemm.hip, dma2_perlane)
__device__ __forceinline__ void dma1(const void* p, unsigned lds) {
  unsigned keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\t"
      "s_mov_b32 m0, %1\n\t"
      "s_nop 2\n\t"
      "global_load_lds_dwordx4 %2, off\n\t"
      "s_mov_b32 m0, %0"
      : "=&s"(keep)
      : "s"(lds), "v"(p)
      : "memory", "scc");
}

// rows [r0, r0 + 32) of a strided [N][64] matrix -> a [32][64] LDS block image (swizzled like the big images, local rows);
// wave w moves slab w (rows 8 w .. 8 w + 7); rows >= nrows repeat row nrows - 1
__device__ __forceinline__ void dma_block(char* blk, const __bf16* src, size_t row_stride, int r0, int nrows, int wave, int lane) {
  const int lr = wave * 8 + (lane >> 3), c = (lane & 7) ^ ((lr >> 1) & 7);
  const __bf16* g = src + (size_t)min(r0 + lr, nrows - 1) * row_stride + c * 8;
  dma1(g, (unsigned)(size_t)LDS_PTR(blk) + (unsigned)wave * 1024u);
}

// DROP (attn_bwd4_drop_kernel): with m = keep / (1 - p) regenerated from the forward's counters, dV = (P m)^T dO and dS = P (dP m - delta);
// delta = rowsum(dO O) as before, O having been formed from the dropped P.  Here the KEY is on the lane and a lane's four registers are four
// QUERY rows, i.e. four counters; the four lanes of a quad hold four consecutive keys of those same rows, so lane p of the quad runs the
// one Philox call of row p and the quad trades words (three DPP quad permutes): one call per lane for four elements, as in the forward.
// (body: csrc/attention_bwd.inc, included once per kernel like the forward's)
__global__ __launch_bounds__(B4_WAVES * 64, 2) void attn_bwd4_kernel(const AttnBwdArgs a) {
#define ATTN_DROP 0
#include "attention_bwd.inc"
#undef ATTN_DROP
}
__global__ __launch_bounds__(B4_WAVES * 64, 2) void attn_bwd4_drop_kernel(const AttnBwdArgs a, const DropKey dkey) {
#define ATTN_DROP 1
#include "attention_bwd.inc"
#undef ATTN_DROP
}

constexpr int FWD_LDS = 2 * FWD_IMG + (DEVIT_ATTN_OUT_ROWS ? FWD_WAVES * 16 * OSLAB_ROW : 0);   // 57344 + 18432: two workgroups per CU

}  // namespace

namespace {

int launch_attn_fwd(const AttnFwdArgs& a, int dtype16, void* stream) {
  static bool attr_set = false;
  if (!attr_set) {
    hipError_t e = hipFuncSetAttribute((const void*)attn_fwd_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, FWD_LDS);
    if (e == hipSuccess)
      e = hipFuncSetAttribute((const void*)attn_fwd_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, FWD_LDS);
    DEVIT_CHECK(e == hipSuccess, DEVIT_ERR_LAUNCH, "devit_attn_fwd: hipFuncSetAttribute: %s", hipGetErrorString(e));
    attr_set = true;
  }
  if (dtype16)
    hipLaunchKernelGGL(attn_fwd_kernel<true>, dim3(a.B * a.H), dim3(FWD_WAVES * 64), FWD_LDS, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(attn_fwd_kernel<false>, dim3(a.B * a.H), dim3(FWD_WAVES * 64), FWD_LDS, (hipStream_t)stream, a);
  DEVIT_LAUNCH_CHECK();
  return DEVIT_OK;
}

int launch_attn_fwd_drop(const AttnFwdArgs& a, const DropKey& dk, void* stream) {
  static bool attr_set = false;
  if (!attr_set) {
    hipError_t e = hipFuncSetAttribute((const void*)attn_fwd_drop_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, FWD_LDS);
    DEVIT_CHECK(e == hipSuccess, DEVIT_ERR_LAUNCH, "devit_attn_fwd_drop: hipFuncSetAttribute: %s", hipGetErrorString(e));
    attr_set = true;
  }
  hipLaunchKernelGGL(attn_fwd_drop_kernel<false>, dim3(a.B * a.H), dim3(FWD_WAVES * 64), FWD_LDS, (hipStream_t)stream, a, dk);
  DEVIT_LAUNCH_CHECK();
  return DEVIT_OK;
}

int launch_attn_bwd_drop(const AttnBwdArgs& a, const DropKey& dk, void* stream) {
  static bool attr_set = false;
  if (!attr_set) {
    hipError_t e = hipFuncSetAttribute((const void*)attn_bwd4_drop_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, BWD4_LDS);
    DEVIT_CHECK(e == hipSuccess, DEVIT_ERR_LAUNCH, "devit_attn_bwd_drop: hipFuncSetAttribute: %s", hipGetErrorString(e));
    attr_set = true;
  }
  hipLaunchKernelGGL(attn_bwd4_drop_kernel, dim3(a.B * a.H), dim3(B4_WAVES * 64), BWD4_LDS, (hipStream_t)stream, a, dk);
  DEVIT_LAUNCH_CHECK();
  return DEVIT_OK;
}

int launch_attn_bwd(const AttnBwdArgs& a, void* stream) {
  static bool attr_set = false;
  if (!attr_set) {
    hipError_t e = hipFuncSetAttribute((const void*)attn_bwd4_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, BWD4_LDS);
    DEVIT_CHECK(e == hipSuccess, DEVIT_ERR_LAUNCH, "devit_attn_bwd: hipFuncSetAttribute: %s", hipGetErrorString(e));
    attr_set = true;
  }
  hipLaunchKernelGGL(attn_bwd4_kernel, dim3(a.B * a.H), dim3(B4_WAVES * 64), BWD4_LDS, (hipStream_t)stream, a);
  DEVIT_LAUNCH_CHECK();
  return DEVIT_OK;
}

bool al16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

// what the launch observer is told about an attention call: B * N token rows, B * NQ query rows (0: the packed-qkv entry points), H * 64 features
devit_launch_info attn_info(const char* name, int B, int N, int NQ, int H, bool dqkv_add = false) {
  devit_launch_info i = {name};
  i.rows = B * N; i.q_rows = B * NQ; i.width = H * HD;
  i.has = dqkv_add ? DEVIT_HAS_DQKV_ADD : 0;
  return i;
}

}  // namespace

extern "C" int devit_attn_fwd(const void* qkv, void* out, float* lse, const float* head_gate, int B, int N, int H,
                              int head_dim, float scale, int dtype16, void* stream) {
  DEVIT_CHECK(qkv && out && (dtype16 == 0 || dtype16 == 1), DEVIT_ERR_ARG, "devit_attn_fwd: bad argument");
  DEVIT_CHECK(head_dim == HD && N > 0 && N <= MAXT * 16 && B > 0 && H > 0, DEVIT_ERR_SHAPE,
              "devit_attn_fwd: needs head_dim == 64 and N <= 208 (got hd=%d N=%d)", head_dim, N);
  const int D = H * HD;
  const __bf16* p = (const __bf16*)qkv;
  AttnFwdArgs a{p, p + D, p + 2 * D, (__bf16*)out, lse, head_gate, B, N, N, H, 3 * D, 3 * D, scale};
  return devit_observed(stream, [&] { return attn_info("devit_attn_fwd", B, N, 0, H); }, [&] { return launch_attn_fwd(a, dtype16, stream); });
}

extern "C" int devit_attn_fwd_rows(const void* q, int q_ld, const void* kv, int kv_ld, void* out, float* lse,
                                   const float* head_gate, int B, int NQ, int N, int H, int head_dim, float scale,
                                   int dtype16, void* stream) {
  DEVIT_CHECK(q && kv && out && (dtype16 == 0 || dtype16 == 1), DEVIT_ERR_ARG, "devit_attn_fwd_rows: bad argument");
  DEVIT_CHECK(head_dim == HD && N > 0 && N <= MAXT * 16 && NQ > 0 && NQ <= N && B > 0 && H > 0, DEVIT_ERR_SHAPE,
              "devit_attn_fwd_rows: needs head_dim == 64, NQ <= N <= 208 (got hd=%d NQ=%d N=%d)", head_dim, NQ, N);
  const int D = H * HD;
  DEVIT_CHECK(q_ld >= D && kv_ld >= 2 * D && q_ld % 8 == 0 && kv_ld % 8 == 0 && al16(q) && al16(kv) && al16(out),
              DEVIT_ERR_ARG, "devit_attn_fwd_rows: q_ld=%d kv_ld=%d / pointers must be 16-byte aligned and hold H*64 (2*H*64) features", q_ld, kv_ld);
  const __bf16* p = (const __bf16*)kv;
  AttnFwdArgs a{(const __bf16*)q, p, p + D, (__bf16*)out, lse, head_gate, B, N, NQ, H, q_ld, kv_ld, scale};
  return devit_observed(stream, [&] { return attn_info("devit_attn_fwd_rows", B, N, NQ, H); }, [&] { return launch_attn_fwd(a, dtype16, stream); });
}

extern "C" int devit_attn_bwd(const void* qkv, const void* out, const void* dout, const float* lse,
                              const float* head_gate, const void* dqkv_add, void* dqkv, int B, int N, int H,
                              int head_dim, float scale, void* stream) {
  DEVIT_CHECK(qkv && out && dout && lse && dqkv, DEVIT_ERR_ARG, "devit_attn_bwd: null pointer");
  DEVIT_CHECK(head_dim == HD && N > 0 && N <= MAXT * 16 && B > 0 && H > 0, DEVIT_ERR_SHAPE,
              "devit_attn_bwd: needs head_dim == 64 and N <= 208 (got hd=%d N=%d)", head_dim, N);
  const int D = H * HD;
  const __bf16* p = (const __bf16*)qkv;
  const __bf16* ad = (const __bf16*)dqkv_add;
  __bf16* d = (__bf16*)dqkv;
  AttnBwdArgs a{p, p + D, p + 2 * D, (const __bf16*)out, (const __bf16*)dout, lse, head_gate,
                ad, ad ? ad + D : nullptr, ad ? ad + 2 * D : nullptr, d, d + D, d + 2 * D,
                B, N, N, H, 3 * D, 3 * D, 3 * D, 3 * D, scale};
  return devit_observed(stream, [&] { return attn_info("devit_attn_bwd", B, N, 0, H, dqkv_add != nullptr); }, [&] { return launch_attn_bwd(a, stream); });
}

// The packed entry points with nn.Dropout on the softmax (site 1 of dropout.h, block = the encoder block's index): bf16 only (training).
extern "C" int devit_attn_fwd_drop(const void* qkv, void* out, float* lse, const float* head_gate, int B, int N, int H, int head_dim,
                                   float scale, unsigned long long seed, int block, unsigned thr, float scale_keep, void* stream) {
  DEVIT_CHECK(qkv && out && block >= 0, DEVIT_ERR_ARG, "devit_attn_fwd_drop: bad argument");
  DEVIT_CHECK(head_dim == HD && N > 0 && N <= MAXT * 16 && B > 0 && H > 0, DEVIT_ERR_SHAPE,
              "devit_attn_fwd_drop: needs head_dim == 64 and N <= 208 (got hd=%d N=%d)", head_dim, N);
  const int D = H * HD;
  const __bf16* p = (const __bf16*)qkv;
  AttnFwdArgs a{p, p + D, p + 2 * D, (__bf16*)out, lse, head_gate, B, N, N, H, 3 * D, 3 * D, scale};
  const DropKey dk = drop_key(seed, DROP_SITE_ATTN, block, thr, scale_keep);
  return devit_observed(stream, [&] { return attn_info("devit_attn_fwd_drop", B, N, 0, H); }, [&] { return launch_attn_fwd_drop(a, dk, stream); });
}

extern "C" int devit_attn_bwd_drop(const void* qkv, const void* out, const void* dout, const float* lse, const float* head_gate,
                                   const void* dqkv_add, void* dqkv, int B, int N, int H, int head_dim, float scale,
                                   unsigned long long seed, int block, unsigned thr, float scale_keep, void* stream) {
  DEVIT_CHECK(qkv && out && dout && lse && dqkv && block >= 0, DEVIT_ERR_ARG, "devit_attn_bwd_drop: bad argument");
  DEVIT_CHECK(head_dim == HD && N > 0 && N <= MAXT * 16 && B > 0 && H > 0, DEVIT_ERR_SHAPE,
              "devit_attn_bwd_drop: needs head_dim == 64 and N <= 208 (got hd=%d N=%d)", head_dim, N);
  const int D = H * HD;
  const __bf16* p = (const __bf16*)qkv;
  const __bf16* ad = (const __bf16*)dqkv_add;
  __bf16* d = (__bf16*)dqkv;
  AttnBwdArgs a{p, p + D, p + 2 * D, (const __bf16*)out, (const __bf16*)dout, lse, head_gate,
                ad, ad ? ad + D : nullptr, ad ? ad + 2 * D : nullptr, d, d + D, d + 2 * D,
                B, N, N, H, 3 * D, 3 * D, 3 * D, 3 * D, scale};
  const DropKey dk = drop_key(seed, DROP_SITE_ATTN, block, thr, scale_keep);
  return devit_observed(stream, [&] { return attn_info("devit_attn_bwd_drop", B, N, 0, H, dqkv_add != nullptr); },
                        [&] { return launch_attn_bwd_drop(a, dk, stream); });
}

extern "C" int devit_attn_bwd_rows(const void* q, int q_ld, const void* kv, int kv_ld, const void* out, const void* dout,
                                   const float* lse, const float* head_gate, void* dq, int dq_ld, void* dkv, int dkv_ld,
                                   int B, int NQ, int N, int H, int head_dim, float scale, void* stream) {
  DEVIT_CHECK(q && kv && out && dout && lse && dq && dkv, DEVIT_ERR_ARG, "devit_attn_bwd_rows: null pointer");
  DEVIT_CHECK(head_dim == HD && N > 0 && N <= MAXT * 16 && NQ > 0 && NQ <= N && B > 0 && H > 0, DEVIT_ERR_SHAPE,
              "devit_attn_bwd_rows: needs head_dim == 64, NQ <= N <= 208 (got hd=%d NQ=%d N=%d)", head_dim, NQ, N);
  const int D = H * HD;
  DEVIT_CHECK(q_ld >= D && dq_ld >= D && kv_ld >= 2 * D && dkv_ld >= 2 * D && q_ld % 8 == 0 && kv_ld % 8 == 0 &&
                  dq_ld % 8 == 0 && dkv_ld % 8 == 0 && al16(q) && al16(kv) && al16(out) && al16(dout) && al16(dq) && al16(dkv),
              DEVIT_ERR_ARG, "devit_attn_bwd_rows: leading dimensions / pointers must be 16-byte aligned and wide enough");
  const __bf16* p = (const __bf16*)kv;
  __bf16* d = (__bf16*)dkv;
  AttnBwdArgs a{(const __bf16*)q, p, p + D, (const __bf16*)out, (const __bf16*)dout, lse, head_gate,
                nullptr, nullptr, nullptr, (__bf16*)dq, d, d + D, B, N, NQ, H, q_ld, kv_ld, dq_ld, dkv_ld, scale};
  return devit_observed(stream, [&] { return attn_info("devit_attn_bwd_rows", B, N, NQ, H); }, [&] { return launch_attn_bwd(a, stream); });
}
