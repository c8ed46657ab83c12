// The 208-row Gram-pair tile under relation.hip (KL between the row softmaxes of F F^T) and qkvce.hip (soft cross-entropy between those of
// X_i X_j^T): one eight-wave workgroup per image holds the teacher's and the student's Gram in registers, takes the row statistics from the
// accumulators, emits S = coef (dP_rows + dP_cols) as bf16 [208][224], and the backward multiplies S by the image's rows.  The two units differ in
// how a row is found in the packed qkv buffer, in the per-row term and in what they keep in LDS; their four __global__ kernels stay their own.
//
// The tile's code lives ONCE, as text: gram_pair_accum.inc (the Gram K loop), gram_pair_stats.inc (row statistics), gram_pair_emit.inc (S) and
// gram_pair_bwd.inc (the backward), each included where it runs and parameterised by the macros its header lists (the pattern of
// cls_loss_kernel.inc).  Not templates: the forward kernels sit at 254 / 256 VGPRs and the relation backward at the 128 its launch bounds allow,
// and a function boundary -- even the same statements inside an always-inline lambda -- gives the optimiser another order of work and these
// kernels other instructions (as policy templates the qkv forward spilled four registers).  As fragments all seven instantiations keep the machine
// code they had as two hand-written copies (profiles/gram_pair_kernel_digests.diff).
#pragma once
#include "devit_common.h"

namespace {

constexpr int GP_ROWS = 208;              // 13 MFMA tiles: the attention kernels' row limit
constexpr int GP_TILES = GP_ROWS / 16;
constexpr int GP_SLD = 224;               // S row stride: seven 32-wide K steps of the backward product
constexpr int GP_STRIDE = 144;            // bytes per LDS row: 64 16-bit elements + 16 bytes, so that 16 rows' 16-byte reads spread over the banks
constexpr int GP_STAGE = GP_ROWS * GP_STRIDE;      // one forward stage: a 64-wide K chunk of the image's 208 rows
constexpr int GP_SEGS = GP_ROWS * 8;      // 16-byte pieces of one K chunk
constexpr int GP_BSTAGE = GP_SLD * GP_STRIDE;      // one backward stage: the chunk's rows out to the K tail of S
constexpr int GP_BSEGS = GP_SLD * 8;

__device__ __forceinline__ float group16_max(float v) {
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ float group16_sum(float v) {
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ---- row addressing: where (row r, 64-wide chunk c) of the component at column `col` starts in an image's packed rows (row stride ld) -----------
// A policy is the set of macros a unit hands the fragments: the loaders' lane values (computed once, so that the K loops hold no multiplication
// or division) and the address of the thread's u-th 16-byte piece: piece tid % 8 of row tid / 8 + 64 u.
//   direct    : r ld + col + 64 c, the head-concatenated rows of the buffer itself (relation.hip defines it beside its kernels).
//   chunk map : a table in LDS, entry g = r H + c holds token | head << 8, offset = token ld + col + 64 head.  view: the reference's
//               `.view(B, N, H * 64)` of a [B, H, N, 64] tensor, head g / N, token g % N; otherwise head c, token r (the identity map).
constexpr int GP_MAP = GP_ROWS * 16;      // table entries: 208 rows x up to 16 chunks
__device__ __forceinline__ void fill_chunk_map(unsigned* tab, int N, int H, bool view, int tid) {
  for (unsigned e = tid; e < (unsigned)(N * H); e += 512) {
    const unsigned q = e / (unsigned)(view ? N : H), r = e - q * (unsigned)(view ? N : H);
    tab[e] = view ? (r | q << 8) : (q | r << 8);
  }
}
__device__ __forceinline__ unsigned chunk_off(unsigned entry, int ld, int col) {
  return (entry & 255u) * (unsigned)ld + (entry >> 8) * 64u + (unsigned)col;
}
// the thread's piece u under the chunk map; row0H = (tid / 8) H is the lane value
#define GP_CHUNK_MAP_PIECE(img, tab, row0H, H, u, c, ld, col) ((img) + (chunk_off((tab)[(row0H) + 64 * (u) * (H) + (c)], ld, col) + (tid & 7) * 8))

inline bool gram_pair_shape_ok(int B, int N, int D, int ld) {
  return B > 0 && N > 0 && N <= GP_ROWS && D > 0 && D <= 1024 && D % 64 == 0 && ld >= 3 * D && ld % 8 == 0;
}

}  // namespace
