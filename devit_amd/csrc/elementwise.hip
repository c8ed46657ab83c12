// HBM-bound helper kernels of the DeViT path: patch im2row, token assembly, casts, column sums
// (bias gradients), embedding backward, small strided f32 GEMM (classifier heads).
#include "det.h"
#include "devit_common.h"

namespace {

// ---- im2row: image f32 [B,3,S,S] -> bf16 rows [B*T][768], k = c*256 + kh*16 + kw, token t = py*G + px -------------
// (timm PatchEmbed Conv2d(3,D,16,16) as a GEMM operand; models/de_vit.py:166-168,258)
// The patch-cutting kernels are templates on G = S / 16 (devit_common.h: 2 .. 14, T = G * G tokens): a 16-byte output chunk is 8 consecutive
// pixels of one image row, at a float offset that is a multiple of 8 for every S % 16 == 0, so the two 16-byte loads stay aligned; G = 14 is
// the 224-pixel kernel as it always was.
template <int G>
__global__ __launch_bounds__(256) void im2row_kernel(const float* img, __bf16* rows, int B, int f16) {
  constexpr int T = G * G, S = G * 16;
  const int total = B * T * 96;  // 16-byte (8-element) output chunks
  for (int idx = blockIdx.x * 256 + threadIdx.x; idx < total; idx += gridDim.x * 256) {
    const int k8 = idx % 96, row = idx / 96;
    const int b = row / T, t = row % T, py = t / G, px = t % G;
    const int c = k8 >> 5, kh = (k8 >> 1) & 15, kw0 = (k8 & 1) * 8;
    const float* src = img + (((size_t)b * 3 + c) * S + py * 16 + kh) * S + px * 16 + kw0;
    const f32x4 v0 = *(const f32x4*)src, v1 = *(const f32x4*)(src + 4);
    *(bf16x8*)(rows + (size_t)idx * 8) = f16 ? cvt8<true>(v0, v1) : cvt8<false>(v0, v1);
  }
}

// ---- Mixup / CutMix fused into im2row (engine.py:65-66 -> timm Mixup(mode='batch') -> patch_embed, de_vit.py:258) ---
// rows[b] = patches of   mode 1: lam * img[b] + (1 - lam) * img[B-1-b]        (x.mul_(lam).add_(x.flip(0) * (1 - lam)))
//                        mode 2: img[b] with the box [y0,y1) x [x0,x1) taken from img[B-1-b]   (x[:, :, yl:yh, xl:xh] = ...)
//                        mode 0: img[b]
// One read of the fp32 batch (each image twice), bf16 patch rows out; the mixed fp32 batch never exists.  The products
// and the sum are rounded separately (no FMA contraction), as the reference's tensor ops round them.
struct MixArgs {
  const float* img;
  __bf16* rows;         // bf16 patch rows (student) or NULL
  __bf16* rows_f16;     // the same values as IEEE f16 (f16 teacher) or NULL
  int B, mode, y0, y1, x0, x1;
  float lam, oml;      // f32(lam), f32(1 - lam) with the subtraction done in double on the host, as torch does for a python scalar
};
template <int G>
__global__ __launch_bounds__(256) void mix_im2row_kernel(const MixArgs a) {
#pragma clang fp contract(off)   // x * lam + flip * (1 - lam) as three rounded operations (hipcc would fuse a multiply-add)
  constexpr int T = G * G, S = G * 16;
  const int total = a.B * T * 96;
  const float lam = a.lam, oml = a.oml;
  for (int idx = blockIdx.x * 256 + threadIdx.x; idx < total; idx += gridDim.x * 256) {
    const int k8 = idx % 96, row = idx / 96;
    const int b = row / T, t = row % T, py = t / G, px = t % G;
    const int c = k8 >> 5, kh = (k8 >> 1) & 15, kw0 = (k8 & 1) * 8;
    const int y = py * 16 + kh, x = px * 16 + kw0;
    const size_t off = ((size_t)c * S + y) * S + x;
    const float* src = a.img + (size_t)b * 3 * S * S + off;
    const float* flp = a.img + (size_t)(a.B - 1 - b) * 3 * S * S + off;
    float v[8];
    *(f32x4*)v = *(const f32x4*)src;
    *(f32x4*)(v + 4) = *(const f32x4*)(src + 4);
    if (a.mode == 1) {
      float w[8];
      *(f32x4*)w = *(const f32x4*)flp;
      *(f32x4*)(w + 4) = *(const f32x4*)(flp + 4);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float p0 = v[e] * lam, p1 = w[e] * oml;
        v[e] = p0 + p1;
      }
    } else if (a.mode == 2 && y >= a.y0 && y < a.y1 && x + 8 > a.x0 && x < a.x1) {
      float w[8];
      *(f32x4*)w = *(const f32x4*)flp;
      *(f32x4*)(w + 4) = *(const f32x4*)(flp + 4);
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = (x + e >= a.x0 && x + e < a.x1) ? w[e] : v[e];
    }
    const f32x4 lo = {v[0], v[1], v[2], v[3]}, hi = {v[4], v[5], v[6], v[7]};
    if (a.rows) *(bf16x8*)(a.rows + (size_t)idx * 8) = cvt8<false>(lo, hi);
    if (a.rows_f16) *(bf16x8*)(a.rows_f16 + (size_t)idx * 8) = cvt8<true>(lo, hi);
  }
}

// targets[b][c] = lam * smooth(y[b])[c] + (1 - lam) * smooth(y[B-1-b])[c],  smooth(y)[c] = eps / C + (c == y) * (1 - eps)
// (timm mixup_target / one_hot; distill_sub.py:315-318)
__global__ __launch_bounds__(256) void mix_targets_kernel(const long long* y, float* out, int B, int C, float lam, float oml,
                                                          float off, float on) {
#pragma clang fp contract(off)
  const int total = B * C;
  for (int idx = blockIdx.x * 256 + threadIdx.x; idx < total; idx += gridDim.x * 256) {
    const int b = idx / C, c = idx % C;
    const float t1 = (int)y[b] == c ? on : off, t2 = (int)y[B - 1 - b] == c ? on : off;
    const float p0 = t1 * lam, p1 = t2 * oml;
    out[idx] = p0 + p1;
  }
}

// ---- the same stage with one (mode, lam, box) per sample (timm Mixup mode='elem' / 'pair': _mix_elem / _mix_pair) ----------
// blockIdx.y picks the sample, so its table entry is uniform over the workgroup: a mode 0 sample never loads its partner (B-1-b), a
// cutmix sample loads it only for the 8-element chunks that meet the box.  Consecutive grid rows are the two samples of a pair
// (0, B-1, 1, B-2, ...), so that the workgroups that read an image as their own and as their partner's are dispatched next to
// each other (measured against sample order, profiles/r12_b_mix_table_cost.json "grid_mapping_us": 71.5 us against 91.0 us for an
// all-mixup table at B = 256).  1 - lam is formed HERE in fp32 from the fp32 lam (timm: lam_batch is float32, and 1 - lam on a
// np.float32 stays float32) -- mix_im2row_kernel above gets f32(1 - lam) from a double subtraction on the host, as timm's batch
// mode does; both stay as they are.  No address depends on what the table holds: only selects and branches do, so any table bytes
// are memory-safe (the host validates the values before it uploads them).
struct MixTableArgs {
  const float* img;
  __bf16* rows;         // bf16 patch rows or NULL
  __bf16* rows_f16;     // the same values as IEEE f16 or NULL
  float* img_out;       // the mixed batch as fp32 images [B,3,S,S] (f32 models) or NULL; never img itself
  const devit_mix_sample* table;
  int B;
};
template <int G>
__global__ __launch_bounds__(256) void mix_im2row_table_kernel(const MixTableArgs a) {
#pragma clang fp contract(off)   // x * lam + flip * (1 - lam) as three rounded operations, and 1 - lam a fourth
  constexpr int T = G * G, S = G * 16;
  const int b = (blockIdx.y & 1) ? a.B - 1 - (int)(blockIdx.y >> 1) : (int)(blockIdx.y >> 1);
  const devit_mix_sample s = a.table[b];
  const float lam = s.lam, oml = 1.0f - lam;
  const size_t img_b = (size_t)b * 3 * S * S, img_p = (size_t)(a.B - 1 - b) * 3 * S * S;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < T * 96; i += gridDim.x * 256) {
    const int k8 = i % 96, t = i / 96, py = t / G, px = t % G;
    const int c = k8 >> 5, kh = (k8 >> 1) & 15, kw0 = (k8 & 1) * 8;
    const int y = py * 16 + kh, x = px * 16 + kw0;
    const size_t off = ((size_t)c * S + y) * S + x;
    const float* src = a.img + img_b + off;
    const float* flp = a.img + img_p + off;
    float v[8];
    *(f32x4*)v = *(const f32x4*)src;
    *(f32x4*)(v + 4) = *(const f32x4*)(src + 4);
    if (s.mode == 1) {
      float w[8];
      *(f32x4*)w = *(const f32x4*)flp;
      *(f32x4*)(w + 4) = *(const f32x4*)(flp + 4);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float p0 = v[e] * lam, p1 = w[e] * oml;
        v[e] = p0 + p1;
      }
    } else if (s.mode == 2 && y >= s.y0 && y < s.y1 && x + 8 > s.x0 && x < s.x1) {
      float w[8];
      *(f32x4*)w = *(const f32x4*)flp;
      *(f32x4*)(w + 4) = *(const f32x4*)(flp + 4);
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = (x + e >= s.x0 && x + e < s.x1) ? w[e] : v[e];
    }
    const f32x4 lo = {v[0], v[1], v[2], v[3]}, hi = {v[4], v[5], v[6], v[7]};
    const size_t chunk = (size_t)b * (T * 96) + i;
    if (a.rows) *(bf16x8*)(a.rows + chunk * 8) = cvt8<false>(lo, hi);
    if (a.rows_f16) *(bf16x8*)(a.rows_f16 + chunk * 8) = cvt8<true>(lo, hi);
    if (a.img_out) {
      float* dst = a.img_out + img_b + off;
      *(f32x4*)dst = lo;
      *(f32x4*)(dst + 4) = hi;
    }
  }
}

// targets[b][c] = lam_b * smooth(y[b])[c] + (1.0f - lam_b) * smooth(y[B-1-b])[c]   (timm mixup_target with a [B,1] float32 lam)
__global__ __launch_bounds__(256) void mix_targets_table_kernel(const long long* y, float* out, const devit_mix_sample* table, int B,
                                                                int C, float off, float on) {
#pragma clang fp contract(off)
  const int total = B * C;
  for (int idx = blockIdx.x * 256 + threadIdx.x; idx < total; idx += gridDim.x * 256) {
    const int b = idx / C, c = idx % C;
    const float lam = table[b].lam, oml = 1.0f - lam;
    const float t1 = (int)y[b] == c ? on : off, t2 = (int)y[B - 1 - b] == c ? on : off;
    const float p0 = t1 * lam, p1 = t2 * oml;
    out[idx] = p0 + p1;
  }
}

// ---- x[b, t] = token_t + pos[t] for the extra (cls / dist) tokens: models/de_vit.py:259-264 ----------
__global__ __launch_bounds__(256) void embed_tokens_kernel(const float* cls, const float* dist, const float* pos,
                                                           float* x, int B, int T, int D, int ntok) {
  const int total = B * ntok * D;
  for (int idx = blockIdx.x * 256 + threadIdx.x; idx < total; idx += gridDim.x * 256) {
    const int d = idx % D, t = (idx / D) % ntok, b = idx / (D * ntok);
    const float tok = t == 0 ? cls[d] : dist[d];
    x[((size_t)b * T + t) * D + d] = tok + pos[(size_t)t * D + d];
  }
}

// ---- f32 -> bf16 cast (weights, once per optimizer step) ----------------------------------------------
__global__ __launch_bounds__(256) void cast_bf16_kernel(const float* src, __bf16* dst, size_t n, int f16) {
  const size_t n8 = n / 8;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n8; i += (size_t)gridDim.x * 256) {
    const f32x4 a = *(const f32x4*)(src + i * 8), b = *(const f32x4*)(src + i * 8 + 4);
    *(bf16x8*)(dst + i * 8) = f16 ? cvt8<true>(a, b) : cvt8<false>(a, b);
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 7)) {
    const float v = src[n8 * 8 + threadIdx.x];
    if (f16) ((_Float16*)dst)[n8 * 8 + threadIdx.x] = (_Float16)v;
    else dst[n8 * 8 + threadIdx.x] = f2bf(v);
  }
}

// ---- f32 [M][D] -> bf16 with an optional per-sample row scale (DropPath) -------------------------------
__global__ __launch_bounds__(256) void scale_cast_kernel(const float* src, __bf16* dst, const float* rowscale,
                                                         int rows_per_scale, int M, int D) {
  const size_t total = (size_t)M * D / 4;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int row = (int)(i * 4 / D);
    const float sc = rowscale ? rowscale[row / rows_per_scale] : 1.0f;
    const f32x4 v = *(const f32x4*)(src + i * 4) * sc;
    bf16x4 o = {f2bf(v[0]), f2bf(v[1]), f2bf(v[2]), f2bf(v[3])};
    *(bf16x4*)(dst + i * 4) = o;
  }
}

// ---- the first ntok rows of every image from one strided matrix into another (devit_token_rows_copy): 16-byte vectors, strides in bytes ----
struct TokenRowsArgs {
  const char* src;
  char* dst;
  size_t src_image, src_row, dst_image, dst_row;
  int ntok, vecs;           // vectors per row
  size_t total;             // B * ntok * vecs
};
template <bool ADD>
__global__ __launch_bounds__(256) void token_rows_copy_kernel(const TokenRowsArgs a) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < a.total; i += (size_t)gridDim.x * 256) {
    const size_t r = i / a.vecs, b = r / a.ntok;
    const size_t v = i - r * a.vecs, t = r - b * a.ntok;
    const f32x4 s = *(const f32x4*)(a.src + b * a.src_image + t * a.src_row + v * 16);
    f32x4* d = (f32x4*)(a.dst + b * a.dst_image + t * a.dst_row + v * 16);
    *d = ADD ? *d + s : s;
  }
}

// ---- column sums of a bf16 [M][ld] matrix (bias gradients): partial[chunk][N] -------------------------
__global__ __launch_bounds__(256) void colsum_bf16_kernel(const __bf16* y, int M, int N, int ld, int row_group,
                                                          int row_skip, float* partial) {
  __shared__ float red[8][256];
  const int cg = threadIdx.x & 31, rl = threadIdx.x >> 5;
  const int col = (blockIdx.x * 32 + cg) * 8;
  const int chunk = blockIdx.y, nchunk = gridDim.y;
  const int r0 = (int)((long long)M * chunk / nchunk), r1 = (int)((long long)M * (chunk + 1) / nchunk);
  float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (col < N) {
    auto prow = [&](int r) { return row_group > 0 ? (size_t)r + row_skip * (r / row_group + 1) : (size_t)r; };
    int r = r0 + rl;
    for (; r + 24 < r1; r += 32) {      // four independent 16-byte loads in flight per thread
      bf16x8 v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = load_stream((const bf16x8*)(y + prow(r + 8 * u) * ld + col));
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] += bf2f(v[u][e]);
    }
    for (; r < r1; r += 8) {
      const bf16x8 v = *(const bf16x8*)(y + prow(r) * ld + col);
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] += bf2f(v[e]);
    }
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) red[rl][cg * 8 + e] = acc[e];
  __syncthreads();
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c < N) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) s += red[i][threadIdx.x];
    partial[(size_t)chunk * N + c] = s;
  }
}

__global__ __launch_bounds__(256) void sum_partials_kernel(const float* partial, int nparts, int ncols, float* out,
                                                           int accumulate) {
  __shared__ float red[8][32];
  const int cl = threadIdx.x & 31, grp = threadIdx.x >> 5;
  const int c = blockIdx.x * 32 + cl;
  float s = 0.f;
  if (c < ncols)
    for (int p = grp; p < nparts; p += 8) s += partial[(size_t)p * ncols + c];
  red[grp][cl] = s;
  __syncthreads();
  if (grp == 0 && c < ncols) {
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) t += red[i][cl];
    out[c] = accumulate ? out[c] + t : t;
  }
}

// ---- embedding backward: dpos[t][d] = sum_b dx[b][t][d]; bf16 copy of dx for the patch wgrad ------------
// gridDim.y slices of the batch per (t, d4) column, four independent 16-byte loads in flight, partial sums combined by
// fp32 atomics into a zeroed / accumulating dpos (8 adds per address).  (One thread per column walking all 256 images
// with one load in flight: 74 workgroups, 1.1 TB/s.)
#define EMBED_BWD_KERNEL embed_bwd_kernel
#define EMBED_BWD_DET 0
#include "embed_bwd_kernel.inc"
#undef EMBED_BWD_KERNEL
#undef EMBED_BWD_DET
#define EMBED_BWD_KERNEL embed_bwd_det_kernel
#define EMBED_BWD_DET 1
#include "embed_bwd_kernel.inc"
#undef EMBED_BWD_KERNEL
#undef EMBED_BWD_DET
// dcls / ddist / dbias from dpos (tiny)
__global__ __launch_bounds__(256) void embed_bwd_tail_kernel(const float* dpos, int T, int D, int ntok, float* dcls,
                                                             float* ddist, float* dbias, int accumulate) {
  const int d = blockIdx.x * 256 + threadIdx.x;
  if (d >= D) return;
  float s = 0.f;
  for (int t = ntok; t < T; ++t) s += dpos[(size_t)t * D + d];
  // NOTE: dpos already holds the accumulated value when accumulate != 0, so the tail always overwrites
  dbias[d] = s;
  dcls[d] = dpos[d];
  if (ddist) ddist[d] = dpos[(size_t)D + d];
  (void)accumulate;
}

// ---- small strided f32 GEMM: C[m][n] = sum_k A[m*sam + k*sak] * B[n*sbn + k*sbk] (+ bias[n]) ------------
// classifier heads (models/de_vit.py:317) and their backward.  Eight lanes per output element, lane p taking
// k = p, p + 8, ... (adjacent lanes read adjacent k: 32-byte pieces of both operand rows), eight independent loads in
// flight per operand and trip, fp32 fmaf partial sums combined by three xor-shuffles.  (One thread per output with a
// serial K loop was a 48 us latency chain at 6400 outputs x K = 384: 25 workgroups on a 256-CU device.)
__global__ __launch_bounds__(256) void sgemm_small_kernel(const float* A, long long sam, long long sak, const float* B,
                                                          long long sbn, long long sbk, const float* bias, float* C,
                                                          int ldc, int M, int N, int K, float alpha, int accumulate) {
  const long long total = (long long)M * N;
  const int part = threadIdx.x & 7;
  for (long long idx = ((long long)blockIdx.x * 256 + threadIdx.x) >> 3; idx < ((total + 31) & ~31ll);
       idx += ((long long)gridDim.x * 256) >> 3) {
    const bool live = idx < total;                       // whole waves stay in the loop: the shuffles need every lane
    const long long id = live ? idx : total - 1;
    const int n = (int)(id % N), m = (int)(id / N);
    const float* a = A + m * sam;
    const float* b = B + n * sbn;
    float s = 0.f;
    int k = part;
    for (; k + 56 < K; k += 64) {
      float av[8], bv[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) { av[u] = a[(k + 8 * u) * sak]; bv[u] = b[(k + 8 * u) * sbk]; }
#pragma unroll
      for (int u = 0; u < 8; ++u) s = fmaf(av[u], bv[u], s);
    }
    for (; k < K; k += 8) s = fmaf(a[k * sak], b[k * sbk], s);
    s += __shfl_xor(s, 1, 64);
    s += __shfl_xor(s, 2, 64);
    s += __shfl_xor(s, 4, 64);
    if (live && part == 0) {
      s = s * alpha + (bias ? bias[n] : 0.f);
      float* c = C + (size_t)m * ldc + n;
      *c = accumulate ? *c + s : s;
    }
  }
}

inline int grid_for(size_t work_items, int cap = 2048) {
  size_t g = (work_items + 255) / 256;
  return (int)(g < 1 ? 1 : (g > (size_t)cap ? cap : g));
}

}  // namespace

// the grid-stride kernels index chunks with an int: B * T * 96 plus one grid stride must fit
inline bool chunks_fit(int B, int G) { return (size_t)B * G * G * 96 <= 0x7fffffffu - 4096u * 256u; }

extern "C" int devit_im2row_bf16(const float* img, void* rows, int B, int C, int H, int W, int patch, int dtype16,
                                 void* stream) {
  DEVIT_CHECK(img && rows && (dtype16 == 0 || dtype16 == 1), DEVIT_ERR_ARG, "devit_im2row_bf16: bad argument");
  const int G = devit_patch_grid(C, H, W, patch);
  DEVIT_CHECK(G > 0 && B > 0, DEVIT_ERR_SHAPE, "devit_im2row_bf16: only " DEVIT_PATCH_SIZES_MSG " (got %dx%dx%d / %d)", C, H, W, patch);
  DEVIT_CHECK(chunks_fit(B, G), DEVIT_ERR_SHAPE, "devit_im2row_bf16: B = %d is too many %dx%d images for one launch", B, H, W);
#define DEVIT_LAUNCH_G(G_)                                                                                                    \
  hipLaunchKernelGGL(im2row_kernel<G_>, dim3(grid_for((size_t)B * (G_ * G_) * 96, 4096)), dim3(256), 0, (hipStream_t)stream, img, \
                     (__bf16*)rows, B, dtype16)
  DEVIT_FOR_PATCH_GRID(G, DEVIT_LAUNCH_G)
#undef DEVIT_LAUNCH_G
  DEVIT_LAUNCH_CHECK();
  return DEVIT_OK;
}

extern "C" int devit_mix_im2row_bf16_sized(const float* img, void* rows, void* rows_f16, int B, int mode, double lam, int y0,
                                           int y1, int x0, int x1, int H, int W, void* stream) {
  DEVIT_CHECK(img && (rows || rows_f16) && B > 0, DEVIT_ERR_ARG, "devit_mix_im2row_bf16: bad argument");
  DEVIT_CHECK(mode >= 0 && mode <= 2, DEVIT_ERR_ARG, "devit_mix_im2row_bf16: mode %d (0 none, 1 mixup, 2 cutmix)", mode);
  const int G = devit_patch_grid(3, H, W, 16);
  DEVIT_CHECK(G > 0, DEVIT_ERR_SHAPE, "devit_mix_im2row_bf16: only " DEVIT_PATCH_SIZES_MSG " (got %dx%d)", H, W);
  DEVIT_CHECK(chunks_fit(B, G), DEVIT_ERR_SHAPE, "devit_mix_im2row_bf16: B = %d is too many %dx%d images for one launch", B, H, W);
  DEVIT_CHECK(mode != 2 || (0 <= y0 && y0 <= y1 && y1 <= H && 0 <= x0 && x0 <= x1 && x1 <= W), DEVIT_ERR_ARG,
              "devit_mix_im2row_bf16: box [%d,%d) x [%d,%d) outside %dx%d", y0, y1, x0, x1, H, W);
  MixArgs a{img, (__bf16*)rows, (__bf16*)rows_f16, B, mode, y0, y1, x0, x1, (float)lam, (float)(1.0 - lam)};
#define DEVIT_LAUNCH_G(G_) \
  hipLaunchKernelGGL(mix_im2row_kernel<G_>, dim3(grid_for((size_t)B * (G_ * G_) * 96, 4096)), dim3(256), 0, (hipStream_t)stream, a)
  DEVIT_FOR_PATCH_GRID(G, DEVIT_LAUNCH_G)
#undef DEVIT_LAUNCH_G
  DEVIT_LAUNCH_CHECK();
  return DEVIT_OK;
}

extern "C" int devit_mix_im2row_bf16(const float* img, void* rows, void* rows_f16, int B, int mode, double lam, int y0,
                                     int y1, int x0, int x1, void* stream) {
  return devit_mix_im2row_bf16_sized(img, rows, rows_f16, B, mode, lam, y0, y1, x0, x1, 224, 224, stream);
}

extern "C" int devit_mix_targets(const long long* labels, float* targets, int B, int C, double lam, double smoothing,
                                 void* stream) {
  DEVIT_CHECK(labels && targets && B > 0 && C > 0, DEVIT_ERR_ARG, "devit_mix_targets: bad argument");
  const double off = smoothing / C, on = 1.0 - smoothing + off;      // timm mixup_target: off / on values in double
  hipLaunchKernelGGL(mix_targets_kernel, dim3(grid_for((size_t)B * C)), dim3(256), 0, (hipStream_t)stream, labels, targets, B,
                     C, (float)lam, (float)(1.0 - lam), (float)off, (float)on);
  DEVIT_LAUNCH_CHECK();
  return DEVIT_OK;
}

extern "C" int devit_mix_im2row_table_sized(const float* img, void* rows, void* rows_f16, float* img_out, const devit_mix_sample* table,
                                            int B, int H, int W, void* stream) {
  DEVIT_CHECK(img && table && (rows || rows_f16 || img_out), DEVIT_ERR_ARG, "devit_mix_im2row_table: bad argument");
  DEVIT_CHECK(B > 0 && B <= 65535, DEVIT_ERR_ARG, "devit_mix_im2row_table: B = %d outside 1 .. 65535 (one grid row per sample)", B);
  DEVIT_CHECK(img_out != img, DEVIT_ERR_ARG,
              "devit_mix_im2row_table: img_out is img (a sample's partner is read after the sample may have been written)");
  const int G = devit_patch_grid(3, H, W, 16);
  DEVIT_CHECK(G > 0, DEVIT_ERR_SHAPE, "devit_mix_im2row_table: only " DEVIT_PATCH_SIZES_MSG " (got %dx%d)", H, W);
  // the table's VALUES are not checked here (device memory; reading it would synchronise): no address in the kernel depends on them
  MixTableArgs a{img, (__bf16*)rows, (__bf16*)rows_f16, img_out, table, B};
  // one 8-element chunk per thread (196 * 96 chunks per 224-pixel sample = 73.5 workgroups); a grid-stride over 16 workgroups per sample
  // measured 7 to 11 us slower at B = 256 (profiles/r12_b_mix_table_cost.json, "grid_mapping_us")
#define DEVIT_LAUNCH_G(G_) \
  hipLaunchKernelGGL(mix_im2row_table_kernel<G_>, dim3((G_ * G_ * 96 + 255) / 256, B), dim3(256), 0, (hipStream_t)stream, a)
  DEVIT_FOR_PATCH_GRID(G, DEVIT_LAUNCH_G)
#undef DEVIT_LAUNCH_G
  DEVIT_LAUNCH_CHECK();
  return DEVIT_OK;
}

extern "C" int devit_mix_im2row_table(const float* img, void* rows, void* rows_f16, float* img_out, const devit_mix_sample* table,
                                      int B, void* stream) {
  return devit_mix_im2row_table_sized(img, rows, rows_f16, img_out, table, B, 224, 224, stream);
}

extern "C" int devit_mix_targets_table(const long long* labels, float* targets, const devit_mix_sample* table, int B, int C,
                                       double smoothing, void* stream) {
  DEVIT_CHECK(labels && targets && table && B > 0 && C > 0 && (size_t)B * C <= 0x7fffffffu, DEVIT_ERR_ARG,
              "devit_mix_targets_table: bad argument");
  const double off = smoothing / C, on = 1.0 - smoothing + off;      // as devit_mix_targets
  hipLaunchKernelGGL(mix_targets_table_kernel, dim3(grid_for((size_t)B * C)), dim3(256), 0, (hipStream_t)stream, labels, targets,
                     table, B, C, (float)off, (float)on);
  DEVIT_LAUNCH_CHECK();
  return DEVIT_OK;
}

extern "C" int devit_embed_tokens(const float* cls, const float* dist, const float* pos, float* x, int B, int T, int D,
                                  void* stream) {
  DEVIT_CHECK(cls && pos && x, DEVIT_ERR_ARG, "devit_embed_tokens: null pointer");
  const int ntok = dist ? 2 : 1;
  hipLaunchKernelGGL(embed_tokens_kernel, dim3(grid_for((size_t)B * ntok * D)), dim3(256), 0, (hipStream_t)stream, cls,
                     dist, pos, x, B, T, D, ntok);
  DEVIT_LAUNCH_CHECK();
  return DEVIT_OK;
}

extern "C" int devit_cast_bf16(const float* src, void* dst, size_t n, int dtype16, void* stream) {
  DEVIT_CHECK(src && dst && (dtype16 == 0 || dtype16 == 1), DEVIT_ERR_ARG, "devit_cast_bf16: bad argument");
  DEVIT_CHECK((((uintptr_t)src) & 15) == 0 && (((uintptr_t)dst) & 15) == 0, DEVIT_ERR_ARG, "devit_cast_bf16: alignment");
  hipLaunchKernelGGL(cast_bf16_kernel, dim3(grid_for(n / 8 + 1)), dim3(256), 0, (hipStream_t)stream, src, (__bf16*)dst, n, dtype16);
  DEVIT_LAUNCH_CHECK();
  return DEVIT_OK;
}

extern "C" int devit_scale_cast_bf16(const float* src, void* dst, const float* rowscale, int rows_per_scale, int M,
                                     int D, void* stream) {
  DEVIT_CHECK(src && dst && (!rowscale || rows_per_scale > 0), DEVIT_ERR_ARG, "devit_scale_cast_bf16: bad argument");
  DEVIT_CHECK(D % 4 == 0 && M > 0, DEVIT_ERR_SHAPE, "devit_scale_cast_bf16: D %% 4");
  hipLaunchKernelGGL(scale_cast_kernel, dim3(grid_for((size_t)M * D / 4, 4096)), dim3(256), 0, (hipStream_t)stream, src,
                     (__bf16*)dst, rowscale, rows_per_scale, M, D);
  DEVIT_LAUNCH_CHECK();
  return DEVIT_OK;
}

extern "C" int devit_token_rows_copy(const void* src, int src_rows_per_image, int src_ld, void* dst, int dst_rows_per_image, int dst_ld, int B,
                                     int ntok, int cols, int elem, int add, void* stream) {
  DEVIT_CHECK(src && dst && (elem == 2 || elem == 4) && (!add || elem == 4), DEVIT_ERR_ARG,
              "devit_token_rows_copy: null pointer / elem=%d not 2 or 4 / add=%d on 16-bit elements", elem, add);
  DEVIT_CHECK(B > 0 && ntok > 0 && ntok <= src_rows_per_image && ntok <= dst_rows_per_image && cols > 0 && cols <= src_ld && cols <= dst_ld,
              DEVIT_ERR_SHAPE, "devit_token_rows_copy: B=%d ntok=%d of %d / %d rows per image, cols=%d of ld %d / %d", B, ntok, src_rows_per_image,
              dst_rows_per_image, cols, src_ld, dst_ld);
  const size_t e = (size_t)elem;
  DEVIT_CHECK((((uintptr_t)src) & 15) == 0 && (((uintptr_t)dst) & 15) == 0 && (src_ld * e) % 16 == 0 && (dst_ld * e) % 16 == 0 && (cols * e) % 16 == 0,
              DEVIT_ERR_ARG, "devit_token_rows_copy: pointers, leading dimensions (%d, %d) and cols=%d must be whole 16-byte vectors", src_ld, dst_ld, cols);
  TokenRowsArgs a{(const char*)src, (char*)dst, src_rows_per_image * src_ld * e, src_ld * e, dst_rows_per_image * dst_ld * e, dst_ld * e,
                  ntok, (int)(cols * e / 16), (size_t)B * ntok * (cols * e / 16)};
  if (add)
    hipLaunchKernelGGL(token_rows_copy_kernel<true>, dim3(grid_for(a.total)), dim3(256), 0, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(token_rows_copy_kernel<false>, dim3(grid_for(a.total)), dim3(256), 0, (hipStream_t)stream, a);
  DEVIT_LAUNCH_CHECK();
  return DEVIT_OK;
}

extern "C" size_t devit_colsum_workspace(int M, int N) {
  (void)M;
  return (size_t)64 * N * sizeof(float);
}

extern "C" int devit_colsum_bf16(const void* y, int M, int N, int ld, int row_group, int row_skip, float* out,
                                 int accumulate, void* workspace, size_t workspace_bytes, void* stream) {
  DEVIT_CHECK(y && out && workspace, DEVIT_ERR_ARG, "devit_colsum_bf16: null pointer");
  DEVIT_CHECK(N % 8 == 0 && ld % 8 == 0 && M > 0, DEVIT_ERR_SHAPE, "devit_colsum_bf16: N, ld must be multiples of 8");
  const int nchunk = M >= 64 * 8 ? 64 : 1;
  DEVIT_CHECK(workspace_bytes >= (size_t)nchunk * N * sizeof(float), DEVIT_ERR_ARG, "devit_colsum_bf16: workspace too small");
  hipLaunchKernelGGL(colsum_bf16_kernel, dim3((N + 255) / 256, nchunk), dim3(256), 0, (hipStream_t)stream,
                     (const __bf16*)y, M, N, ld, row_group, row_skip, (float*)workspace);
  DEVIT_LAUNCH_CHECK();
  hipLaunchKernelGGL(sum_partials_kernel, dim3((N + 31) / 32), dim3(256), 0, (hipStream_t)stream,
                     (const float*)workspace, nchunk, N, out, accumulate);
  DEVIT_LAUNCH_CHECK();
  return DEVIT_OK;
}

extern "C" int devit_embed_bwd(const float* dx, int B, int T, int D, int ntok, float* dpos, float* dcls, float* ddist,
                               float* dbias, void* dx_bf16, int accumulate, void* stream) {
  DEVIT_CHECK(dx && dpos && dcls && dbias, DEVIT_ERR_ARG, "devit_embed_bwd: null pointer");
  DEVIT_CHECK(D % 4 == 0 && (ntok == 1 || (ntok == 2 && ddist)), DEVIT_ERR_SHAPE, "devit_embed_bwd: D %% 4, ntok");
  DEVIT_CHECK(accumulate == 0, DEVIT_ERR_ARG, "devit_embed_bwd: accumulate is not supported");
  hipError_t me = hipMemsetAsync(dpos, 0, (size_t)T * D * sizeof(float), (hipStream_t)stream);
  DEVIT_CHECK(me == hipSuccess, DEVIT_ERR_LAUNCH, "devit_embed_bwd: hipMemsetAsync: %s", hipGetErrorString(me));
  const int slices = B >= 64 ? 8 : 1;
  if (slices > 1 && devit_det::on()) {   // deterministic mode (det.h): the slices' sums go to the workspace and are added to dpos in slice order
    float* ws = nullptr;
    const int rc = devit_det::workspace("devit_embed_bwd", (size_t)slices * T * D * sizeof(float), &ws);
    if (rc != DEVIT_OK) return rc;
    hipLaunchKernelGGL(embed_bwd_det_kernel, dim3((T * D / 4 + 255) / 256, slices), dim3(256), 0, (hipStream_t)stream, dx, B, T, D, ws,
                       (__bf16*)dx_bf16);
    DEVIT_LAUNCH_CHECK();
    const int rf = devit_det::fold(ws, slices, (size_t)T * D, 1, T * D, dpos, 0, 1, 0, (hipStream_t)stream);
    if (rf != DEVIT_OK) return rf;
  } else {
    hipLaunchKernelGGL(embed_bwd_kernel, dim3((T * D / 4 + 255) / 256, slices), dim3(256), 0, (hipStream_t)stream, dx, B,
                       T, D, dpos, (__bf16*)dx_bf16);
    DEVIT_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(embed_bwd_tail_kernel, dim3((D + 255) / 256), dim3(256), 0, (hipStream_t)stream,
                     (const float*)dpos, T, D, ntok, dcls, ddist, dbias, accumulate);
  DEVIT_LAUNCH_CHECK();
  return DEVIT_OK;
}

extern "C" int devit_sgemm_small(const float* A, long long sam, long long sak, const float* B, long long sbn,
                                 long long sbk, const float* bias, float* C, int ldc, int M, int N, int K, float alpha,
                                 int accumulate, void* stream) {
  DEVIT_CHECK(A && B && C && M > 0 && N > 0 && K > 0, DEVIT_ERR_ARG, "devit_sgemm_small: bad argument");
  hipLaunchKernelGGL(sgemm_small_kernel, dim3(grid_for((size_t)M * N * 8, 8192)), dim3(256), 0, (hipStream_t)stream, A, sam,
                     sak, B, sbn, sbk, bias, C, ldc, M, N, K, alpha, accumulate);
  DEVIT_LAUNCH_CHECK();
  return DEVIT_OK;
}
