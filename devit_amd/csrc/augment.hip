// Input augmentation (include/devit_hip.h, "Input augmentation"): a resident uint8 image set -> the normalized fp32 batch.
//   augment_coeffs_kernel   PIL's resampling coefficients per (sample, axis, output index), in IEEE double with contraction off,
//                           as int32 into a workspace: [B][2 axes][2 + TAPS][S] = xmin, count, weights (zero behind the count)
//   augment_kernel          one workgroup per (sample, band of 32 output rows): horizontal pass of the source rows the band needs into
//                           LDS as the uint8 intermediate (thread x keeps column x's taps in registers), then the vertical pass, flip,
//                           normalize (a table of the 256 levels per channel, made with the header's two divisions) and erasing out of
//                           LDS into 16-byte stores.  Integer arithmetic up to the normalization.
//   augment_u8_kernel       augment_kernel's two passes and flip, with the uint8 window [B][S][S][3] as the result
//   image_ops_kernel        (header, "Image ops") one workgroup per sample: that window into LDS whole, RandAugment's / ColorJitter's layers applied
//                           there bit for bit as PIL computes them, then normalize and erasing out of LDS; or uint8 to uint8 (devit_image_ops)
//   ragged_coeffs_kernel, ragged_narrow_kernel, ragged_wide_kernel   (header, "Packed sets") the same stage over a packed set of mixed image sizes:
//                           the image's base, H0 and W0 from a directory entry; the narrow kernel is augment_kernel / augment_u8_kernel on that
//                           image, the wide one serves 13 .. 128 taps per axis by streaming source rows into per-column accumulators
// Every source address is clamped and the value masked afterwards (as attention.hip's fetch_rows: no load under a per-element
// condition), every LDS row index is clamped, idx is clamped: no table or index bytes can send an access out of bounds.
#include "devit_common.h"
#include "dropout.h"

namespace {

constexpr int TAPS = DEVIT_AUGMENT_TAPS;
constexpr int PLANES = 2 + TAPS;      // xmin, count, weights
constexpr int BAND = 32;              // output rows per workgroup
constexpr int NROWS = 24;             // source rows of the intermediate held at once (a band is cut into runs that fit; >= TAPS); 16 KB of LDS
constexpr int PITCH = 224;            // bytes per intermediate row: the largest S
constexpr int THREADS = 256;          // >= the largest S: thread x owns output column x in the horizontal pass
constexpr int WEIGHT_ONE = 1 << 22;   // PIL's PRECISION_BITS = 32 - 8 - 2

struct Norm3 {
  float mean[3], std[3];
};

// PIL's bilinear_filter / bicubic_filter (src/libImaging/Resample.c), operation for operation
__device__ __forceinline__ double filter_weight(double x, int cubic) {
#pragma clang fp contract(off)
  if (x < 0.0) x = -x;
  if (cubic) {
    const double a = -0.5;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
  }
  if (x < 1.0) return 1.0 - x;
  return 0.0;
}

// precompute_coeffs + normalize_coeffs_8bpc for one output index xx of an axis of `len` source pixels resized to R
__device__ __forceinline__ void resample_coeffs(int len, int R, int xx, int cubic, int& xmin_out, int& n_out, int (&wq)[TAPS]) {
#pragma clang fp contract(off)
  const double scale = (double)len / (double)R;
  const double fs = scale < 1.0 ? 1.0 : scale;
  const double support = (cubic ? 2.0 : 1.0) * fs;
  const double center = (xx + 0.5) * scale;
  const double ss = 1.0 / fs;
  int xmin = (int)(center - support + 0.5);
  if (xmin < 0) xmin = 0;
  if (xmin > len) xmin = len;                  // (a table the host would have refused: stay inside the box)
  int xmax = (int)(center + support + 0.5);
  if (xmax > len) xmax = len;
  int n = xmax - xmin;
  n = n < 0 ? 0 : (n > TAPS ? TAPS : n);
  double w[TAPS], ww = 0.0;
#pragma unroll
  for (int k = 0; k < TAPS; ++k) {
    w[k] = 0.0;
    if (k < n) {
      w[k] = filter_weight((k + xmin - center + 0.5) * ss, cubic);
      ww += w[k];
    }
  }
#pragma unroll
  for (int k = 0; k < TAPS; ++k) {
    double v = w[k];
    if (k < n && ww != 0.0) v /= ww;
    wq[k] = v < 0 ? (int)(-0.5 + v * (double)WEIGHT_ONE) : (int)(0.5 + v * (double)WEIGHT_ONE);
  }
  xmin_out = xmin;
  n_out = n;
}

__global__ __launch_bounds__(256) void augment_coeffs_kernel(const devit_augment_sample* __restrict__ table, int B, int S,
                                                             int* __restrict__ ws) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= B * 2 * S) return;
  const int j = t % S, axis = (t / S) & 1, b = t / (2 * S);
  const devit_augment_sample* s = table + b;
  const int len = axis ? s->w : s->h, R = axis ? s->Rw : s->Rh, xx = (axis ? s->ox : s->oy) + j, filter = s->filter;
  int xmin = xx, n = 1, wq[TAPS];
#pragma unroll
  for (int k = 0; k < TAPS; ++k) wq[k] = k == 0 ? WEIGHT_ONE : 0;      // unit scale: the pixel itself
  if ((filter == DEVIT_AUG_BILINEAR || filter == DEVIT_AUG_BICUBIC) && len > 0 && R > 0)
    resample_coeffs(len, R, xx, filter == DEVIT_AUG_BICUBIC, xmin, n, wq);
  int* p = ws + (size_t)(b * 2 + axis) * PLANES * S + j;
  p[0] = xmin;
  p[S] = n;
#pragma unroll
  for (int k = 0; k < TAPS; ++k) p[(size_t)(2 + k) * S] = wq[k];
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// Box-Muller halves on one Philox word (the header states the definition): both go through whichever of u and 1 - u is exact in fp32
__device__ __forceinline__ float bm_radius(unsigned w) {
  const unsigned k = w >> 8;
  float L;
  if (k < 0x800000u)
    L = logf(((float)k + 0.5f) * 0x1p-24f);
  else
    L = log1pf(-(((float)(0xFFFFFFu - k) + 0.5f) * 0x1p-24f));
  return sqrtf(-2.0f * L);
}
__device__ __forceinline__ void bm_angle(unsigned w, float& c, float& s) {
  const unsigned k = w >> 8;
  const bool low = k < 0x800000u;
  const float a = ((float)(low ? k : 0xFFFFFFu - k) + 0.5f) * 0x1p-23f;      // 2 u or 2 (1 - u), exact
  c = cospif(a);
  const float sn = sinpif(a);
  s = low ? sn : -sn;
}
__device__ __forceinline__ f32x4 normals4(u32x4 w) {
  float c0, s0, c1, s1;
  const float r0 = bm_radius(w[0]), r1 = bm_radius(w[2]);
  bm_angle(w[1], c0, s0);
  bm_angle(w[3], c1, s1);
  return (f32x4){r0 * c0, r0 * s0, r1 * c1, r1 * s1};
}
__device__ __forceinline__ u32x4 noise_words(unsigned long long N, int c, unsigned g, unsigned k0, unsigned k1) {
  return philox4x32_10((u32x4){(unsigned)N, (unsigned)(N >> 32), DEVIT_AUGMENT_SITE + (unsigned)c, g}, k0, k1);
}

__global__ __launch_bounds__(THREADS) void augment_kernel(const unsigned char* __restrict__ src, int n_img, int H0, int W0,
                                                          const int* __restrict__ idx, const devit_augment_sample* __restrict__ table,
                                                          int S, const int* __restrict__ ws, Norm3 norm, unsigned k0, unsigned k1,
                                                          float* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) unsigned char inter[3][NROWS][PITCH];
  __shared__ int s_ymin[BAND], s_yn[BAND], s_wy[BAND][TAPS];
  __shared__ float s_rand[DEVIT_AUGMENT_MAX_ERASE][3];
  __shared__ float s_norm[3][256];      // the normalized value of every uint8 level: the two divisions are made 768 times per workgroup, not per pixel
  const int tid = threadIdx.x, b = blockIdx.y, r0 = blockIdx.x * BAND, r1 = min(r0 + BAND, S);
  const devit_augment_sample* sp = table + b;
  const int y0 = sp->y0, x0 = sp->x0, flip = sp->flip, n_erase = clampi(sp->n_erase, 0, DEVIT_AUGMENT_MAX_ERASE),
            erase_mode = sp->erase_mode;
  const unsigned long long N = sp->noise_base + (unsigned long long)b;
  const int img = clampi(idx[b], 0, n_img - 1);
  const unsigned char* image = src + (size_t)img * H0 * W0 * 3;
  const int* wsy = ws + (size_t)(b * 2) * PLANES * S;
  const int* wsx = wsy + (size_t)PLANES * S;

  // the band's vertical coefficients -> LDS; column tid's horizontal ones -> registers
  for (int i = tid; i < BAND * PLANES; i += THREADS) {
    const int r = i / PLANES, q = i % PLANES;
    const int v = wsy[(size_t)q * S + min(r0 + r, S - 1)];
    if (q == 0) s_ymin[r] = v;
    else if (q == 1) s_yn[r] = clampi(v, 0, TAPS);
    else s_wy[r][q - 2] = v;
  }
  const int xc = min(tid, S - 1);
  const int xmin_x = wsx[xc];
  int wx[TAPS];
#pragma unroll
  for (int k = 0; k < TAPS; ++k) wx[k] = wsx[(size_t)(2 + k) * S + xc];
  if (erase_mode == DEVIT_AUG_ERASE_RAND && tid < n_erase * 3) {
    const int e = tid / 3, c = tid % 3;
    s_rand[e][c] = normals4(noise_words(N, c, 0x80000000u + (unsigned)e, k0, k1))[0];
  }

  for (int i = tid; i < 3 * 256; i += THREADS) {
    const int c = i >> 8;
    s_norm[c][i & 255] = ((float)(i & 255) / 255.0f - norm.mean[c]) / norm.std[c];
  }

  // vertical pass: a wave takes 64 / nq (row, channel) pairs at a time, lane -> (pair, quad of four output pixels); the divisions are per thread, not per item
  const int nq = S >> 2, lane = tid & 63, per = 64 / nq, sub = lane / nq, xq = lane - sub * nq;
  const int x = xq * 4, xs = flip ? S - 4 - x : x;
  int r = r0;
  while (r < r1) {
    __syncthreads();      // the coefficients are staged; the previous run's intermediate has been read
    const int lo = s_ymin[r - r0];
    int e = r + 1;        // one output row needs at most TAPS <= NROWS source rows: every run advances
    while (e < r1 && s_ymin[e - r0] + s_yn[e - r0] - lo <= NROWS) ++e;
    const int nrows = clampi(s_ymin[e - 1 - r0] + s_yn[e - 1 - r0] - lo, 0, NROWS);

    // horizontal pass: source rows lo .. lo + nrows of the box, output column tid
    if (tid < S) {
      for (int row = 0; row < nrows; ++row) {
        const int sy = y0 + lo + row;
        const bool in_y = sy >= 0 && sy < H0;
        const unsigned char* line = image + (size_t)clampi(sy, 0, H0 - 1) * W0 * 3;
        int a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21;
#pragma unroll
        for (int k = 0; k < TAPS; ++k) {
          const int sx = x0 + xmin_x + k;
          const bool ok = in_y && sx >= 0 && sx < W0;
          const unsigned char* p = line + clampi(sx, 0, W0 - 1) * 3;
          const int p0 = p[0], p1 = p[1], p2 = p[2];
          const int w = ok ? wx[k] : 0;
          a0 += p0 * w;
          a1 += p1 * w;
          a2 += p2 * w;
        }
        inter[0][row][tid] = (unsigned char)clampi(a0 >> 22, 0, 255);
        inter[1][row][tid] = (unsigned char)clampi(a1 >> 22, 0, 255);
        inter[2][row][tid] = (unsigned char)clampi(a2 >> 22, 0, 255);
      }
    }
    __syncthreads();

    // vertical pass, flip, normalize, erase: four output pixels of one row and channel per item
    const int pairs = (e - r) * 3;
    for (int t = (tid >> 6) * per + sub; sub < per && t < pairs; t += (THREADS / 64) * per) {
      const int c = t % 3, yy = r + t / 3;
      const int ymin = s_ymin[yy - r0] - lo, yn = s_yn[yy - r0];
      int acc[4] = {1 << 21, 1 << 21, 1 << 21, 1 << 21};
      for (int k = 0; k < yn; ++k) {
        const unsigned q = *(const unsigned*)&inter[c][clampi(ymin + k, 0, NROWS - 1)][xs];
        const int w = s_wy[yy - r0][k];
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] += (int)((q >> (8 * j)) & 255u) * w;
      }
      f32x4 v;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int u = clampi((flip ? acc[3 - j] : acc[j]) >> 22, 0, 255);
        v[j] = s_norm[c][u];
      }
      unsigned inside = 0;      // bit 4 e + j: pixel j lies in box e
      for (int eb = 0; eb < n_erase; ++eb) {
        const int top = sp->erase[eb][0], left = sp->erase[eb][1], eh = sp->erase[eb][2], ew = sp->erase[eb][3];
        if (yy >= top && yy - top < eh) {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (x + j >= left && x + j - left < ew) inside |= 1u << (4 * eb + j);
        }
      }
      if (inside) {
        f32x4 z = {0.f, 0.f, 0.f, 0.f};
        if (erase_mode == DEVIT_AUG_ERASE_PIXEL) z = normals4(noise_words(N, c, (unsigned)(yy * S + x) >> 2, k0, k1));
#pragma unroll
        for (int eb = 0; eb < DEVIT_AUGMENT_MAX_ERASE; ++eb) {      // later boxes win
          const float zr = erase_mode == DEVIT_AUG_ERASE_RAND ? s_rand[eb][c] : 0.f;
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (inside >> (4 * eb + j) & 1u) v[j] = erase_mode == DEVIT_AUG_ERASE_PIXEL ? z[j] : zr;
        }
      }
      store16_stream(out + (((size_t)b * 3 + c) * S + yy) * S + x, v);
    }
    r = e;
  }
}

// augment_kernel's two passes and flip with the uint8 window [B][S][S][3] as the result (what image_ops_kernel loads): steps 3 and 4 are that kernel's
__global__ __launch_bounds__(THREADS) void augment_u8_kernel(const unsigned char* __restrict__ src, int n_img, int H0, int W0,
                                                             const int* __restrict__ idx, const devit_augment_sample* __restrict__ table,
                                                             int S, const int* __restrict__ ws, unsigned char* __restrict__ out8) {
  __shared__ __attribute__((aligned(16))) unsigned char inter[3][NROWS][PITCH];
  __shared__ int s_ymin[BAND], s_yn[BAND], s_wy[BAND][TAPS];
  const int tid = threadIdx.x, b = blockIdx.y, r0 = blockIdx.x * BAND, r1 = min(r0 + BAND, S);
  const devit_augment_sample* sp = table + b;
  const int y0 = sp->y0, x0 = sp->x0, flip = sp->flip;
  const int img = clampi(idx[b], 0, n_img - 1);
  const unsigned char* image = src + (size_t)img * H0 * W0 * 3;
  const int* wsy = ws + (size_t)(b * 2) * PLANES * S;
  const int* wsx = wsy + (size_t)PLANES * S;

  // the band's vertical coefficients -> LDS; column tid's horizontal ones -> registers
  for (int i = tid; i < BAND * PLANES; i += THREADS) {
    const int r = i / PLANES, q = i % PLANES;
    const int v = wsy[(size_t)q * S + min(r0 + r, S - 1)];
    if (q == 0) s_ymin[r] = v;
    else if (q == 1) s_yn[r] = clampi(v, 0, TAPS);
    else s_wy[r][q - 2] = v;
  }
  const int xc = min(tid, S - 1);
  const int xmin_x = wsx[xc];
  int wx[TAPS];
#pragma unroll
  for (int k = 0; k < TAPS; ++k) wx[k] = wsx[(size_t)(2 + k) * S + xc];
  // vertical pass: a wave takes 64 / nq (row, channel) pairs at a time, lane -> (pair, quad of four output pixels); the divisions are per thread, not per item
  const int nq = S >> 2, lane = tid & 63, per = 64 / nq, sub = lane / nq, xq = lane - sub * nq;
  const int x = xq * 4, xs = flip ? S - 4 - x : x;
  int r = r0;
  while (r < r1) {
    __syncthreads();      // the coefficients are staged; the previous run's intermediate has been read
    const int lo = s_ymin[r - r0];
    int e = r + 1;        // one output row needs at most TAPS <= NROWS source rows: every run advances
    while (e < r1 && s_ymin[e - r0] + s_yn[e - r0] - lo <= NROWS) ++e;
    const int nrows = clampi(s_ymin[e - 1 - r0] + s_yn[e - 1 - r0] - lo, 0, NROWS);

    // horizontal pass: source rows lo .. lo + nrows of the box, output column tid
    if (tid < S) {
      for (int row = 0; row < nrows; ++row) {
        const int sy = y0 + lo + row;
        const bool in_y = sy >= 0 && sy < H0;
        const unsigned char* line = image + (size_t)clampi(sy, 0, H0 - 1) * W0 * 3;
        int a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21;
#pragma unroll
        for (int k = 0; k < TAPS; ++k) {
          const int sx = x0 + xmin_x + k;
          const bool ok = in_y && sx >= 0 && sx < W0;
          const unsigned char* p = line + clampi(sx, 0, W0 - 1) * 3;
          const int p0 = p[0], p1 = p[1], p2 = p[2];
          const int w = ok ? wx[k] : 0;
          a0 += p0 * w;
          a1 += p1 * w;
          a2 += p2 * w;
        }
        inter[0][row][tid] = (unsigned char)clampi(a0 >> 22, 0, 255);
        inter[1][row][tid] = (unsigned char)clampi(a1 >> 22, 0, 255);
        inter[2][row][tid] = (unsigned char)clampi(a2 >> 22, 0, 255);
      }
    }
    __syncthreads();

    // vertical pass and flip: four output pixels of one row and channel per item
    const int pairs = (e - r) * 3;
    for (int t = (tid >> 6) * per + sub; sub < per && t < pairs; t += (THREADS / 64) * per) {
      const int c = t % 3, yy = r + t / 3;
      const int ymin = s_ymin[yy - r0] - lo, yn = s_yn[yy - r0];
      int acc[4] = {1 << 21, 1 << 21, 1 << 21, 1 << 21};
      for (int k = 0; k < yn; ++k) {
        const unsigned q = *(const unsigned*)&inter[c][clampi(ymin + k, 0, NROWS - 1)][xs];
        const int w = s_wy[yy - r0][k];
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] += (int)((q >> (8 * j)) & 255u) * w;
      }
#pragma unroll
      for (int j = 0; j < 4; ++j)
        out8[(((size_t)b * S + yy) * S + x + j) * 3 + c] = (unsigned char)clampi((flip ? acc[3 - j] : acc[j]) >> 22, 0, 255);
    }
    r = e;
  }
}


// ---- image ops (include/devit_hip.h, "Image ops"): one workgroup per sample, the sample's S x S x 3 uint8 image in LDS through every layer --------
constexpr int OPS_THREADS = 512;                                                // 8 waves: 256 VGPRs each, the staged pixels and the fp64 cubic fit without spills
constexpr int OPS_PIX = (224 * 224 + OPS_THREADS - 1) / OPS_THREADS;            // 98 pixels per thread at the largest S, staged as one dword each
constexpr int OPS_FIXED_LDS = 3 * 256 * 4 + 3 * 256 * 4 + 3 * 256 + 3 * 4 * 4 + DEVIT_AUGMENT_MAX_ERASE * 3 * 4 + 16;      // behind the image
static_assert(224 * 224 * 3 + OPS_FIXED_LDS <= 163840, "the image and its tables fit one CU's LDS");

__device__ __forceinline__ int blend8(int d, int u, float f) {
#pragma clang fp contract(off)
  const float df = (float)d;
  const float r = df + f * ((float)u - df);
  if (f >= 0.f && f <= 1.f) return clampi((int)r, 0, 255);
  return r <= 0.f ? 0 : (r >= 255.f ? 255 : clampi((int)r, 0, 255));
}

__device__ __forceinline__ int luma8(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16; }

// ImageFilter.SMOOTH at an inner pixel, channel c
__device__ __forceinline__ int smooth8(const unsigned char* img, int S, int y, int x, int c) {
#pragma clang fp contract(off)
  const float k1 = 1.0f / 13.0f, k5 = 5.0f / 13.0f;
  float acc = 0.f;
#pragma unroll
  for (int j = -1; j <= 1; ++j)
#pragma unroll
    for (int i = -1; i <= 1; ++i) acc = acc + (float)img[((y + j) * S + x + i) * 3 + c] * ((i == 0 && j == 0) ? k5 : k1);
  acc = acc + 0.5f;
  return acc <= 0.f ? 0 : (acc >= 255.f ? 255 : (int)acc);
}

__device__ __forceinline__ double cubic4(double v1, double v2, double v3, double v4, double d) {
#pragma clang fp contract(off)
  const double p1 = v2, p2 = -v1 + v3, p3 = 2 * (v1 - v2) + v3 - v4, p4 = -v1 + v2 - v3 + v4;
  return p1 + d * (p2 + d * (p3 + d * p4));
}

// one output pixel of Image.transform(AFFINE): r | g << 8 | b << 16
__device__ __forceinline__ unsigned affine_pixel(const unsigned char* img, int S, int yo, int xo, const double (&m)[6], bool cubic, unsigned fill) {
#pragma clang fp contract(off)
  const double X = xo + 0.5, Y = yo + 0.5;
  double xin = m[0] * X + m[1] * Y + m[2], yin = m[3] * X + m[4] * Y + m[5];
  if (!(xin >= 0.0 && xin < (double)S && yin >= 0.0 && yin < (double)S)) return fill;      // (a NaN lands here)
  xin -= 0.5;
  yin -= 0.5;
  const double fx = floor(xin), fy = floor(yin);
  const double dx = xin - fx, dy = yin - fy;
  const int x = (int)fx, y = (int)fy;      // -1 .. S - 1
  unsigned px = 0;
  if (cubic) {
    int xc[4], row[4];
    bool ok[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      xc[k] = clampi(x - 1 + k, 0, S - 1) * 3;
      row[k] = clampi(y - 1 + k, 0, S - 1) * S * 3;
      ok[k] = k == 0 || (y - 1 + k >= 0 && y - 1 + k < S);
    }
#pragma unroll 1
    for (int c = 0; c < 3; ++c) {      // (one channel's sixteen taps at a time: the registers belong to the staged pixels)
      double r[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const unsigned char* p = img + row[k] + c;
        const double v = cubic4((double)p[xc[0]], (double)p[xc[1]], (double)p[xc[2]], (double)p[xc[3]], dx);
        r[k] = (k == 0 || ok[k]) ? v : r[k > 0 ? k - 1 : 0];
      }
      const double v = cubic4(r[0], r[1], r[2], r[3], dy);
      px |= (unsigned)(v <= 0.0 ? 0 : (v >= 255.0 ? 255 : (int)v)) << (8 * c);
    }
  } else {
    const int x0 = clampi(x, 0, S - 1) * 3, x1 = clampi(x + 1, 0, S - 1) * 3;
    const int r0 = clampi(y, 0, S - 1) * S * 3, r1 = clampi(y + 1, 0, S - 1) * S * 3;
    const bool ok1 = y + 1 >= 0 && y + 1 < S;
#pragma unroll 1
    for (int c = 0; c < 3; ++c) {
      const double a0 = (double)img[r0 + x0 + c], a1 = (double)img[r0 + x1 + c];
      const double b0 = (double)img[r1 + x0 + c], b1 = (double)img[r1 + x1 + c];
      const double v1 = a0 + (a1 - a0) * dx;
      const double v2 = ok1 ? b0 + (b1 - b0) * dx : v1;
      const double v = v1 + (v2 - v1) * dy;
      px |= (unsigned)clampi((int)v, 0, 255) << (8 * c);
    }
  }
  return px;
}

// One output pixel p of a neighbour op (Sharpness, the affine family) of layer l, read from the image at the start of LDS: r | g << 8 | b << 16
__device__ __forceinline__ unsigned neighbour_pixel(int p, int S, const devit_augment_ops* __restrict__ op, int l) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const unsigned char* img = smem;
  const int y = p / S, x = p - y * S;
  if (op->op[l] == DEVIT_OP_SHARPNESS) {
    const float f = op->factor[l];
    const unsigned char* q = img + p * 3;
    const bool inner = y > 0 && y < S - 1 && x > 0 && x < S - 1;
    const int yc = clampi(y, 1, S - 2), xc = clampi(x, 1, S - 2);
    unsigned v = 0;
#pragma unroll 1
    for (int c = 0; c < 3; ++c) {
      const int u = q[c], s = inner ? smooth8(img, S, yc, xc, c) : u;
      v |= (unsigned)blend8(s, u, f) << (8 * c);
    }
    return v;
  }
  double m[6];
#pragma unroll
  for (int j = 0; j < 6; ++j) m[j] = op->matrix[l][j];
  const unsigned fill = (unsigned)(op->fill[l][0] & 255) | (unsigned)(op->fill[l][1] & 255) << 8 | (unsigned)(op->fill[l][2] & 255) << 16;
  return affine_pixel(img, S, y, x, m, op->filter[l] == DEVIT_AUG_BICUBIC, fill);
}

// FINISH: steps 3 and 4 of "Input augmentation" out of LDS into `out`; else the uint8 image into out8
template <bool FINISH>
__global__ __launch_bounds__(OPS_THREADS) void image_ops_kernel(const unsigned char* __restrict__ in, const devit_augment_ops* __restrict__ ops,
                                                                int S, unsigned char* __restrict__ out8,
                                                                const devit_augment_sample* __restrict__ table, Norm3 norm, unsigned k0,
                                                                unsigned k1, float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, b = blockIdx.x, SS = S * S, n4 = SS * 3 / 4;      // S is a multiple of 16
  unsigned char* img = smem;
  unsigned* img32 = (unsigned*)smem;
  int* s_hist = (int*)(smem + SS * 3);                     // [3][256]: counts, then their exclusive prefix sums
  float* s_norm = (float*)(s_hist + 3 * 256);              // [3][256]
  unsigned char* s_lut = (unsigned char*)(s_norm + 3 * 256);      // [3][256]
  int* s_stat = (int*)(s_lut + 3 * 256);                   // [3][4]: lo, hi, non-empty bins, step
  float* s_rand = (float*)(s_stat + 12);                   // [MAX_ERASE][3]
  int* s_sum = (int*)(s_rand + DEVIT_AUGMENT_MAX_ERASE * 3);
  const devit_augment_ops* op = ops + b;
  const int n_ops = clampi(op->n_ops, 0, DEVIT_AUGMENT_MAX_OPS);
  const int kmax = (SS + OPS_THREADS - 1) / OPS_THREADS;   // <= OPS_PIX

  {
    const unsigned* g = (const unsigned*)(in + (size_t)b * SS * 3);
    for (int i = tid; i < n4; i += OPS_THREADS) img32[i] = g[i];
  }
  __syncthreads();

#pragma unroll 1
  for (int l = 0; l < n_ops; ++l) {
    const int id = op->op[l];
    const float f = op->factor[l];
    const int arg = op->arg[l];
    if (id == DEVIT_OP_COLOR) {                             // pointwise per pixel, in place
      for (int p = tid; p < SS; p += OPS_THREADS) {
        unsigned char* q = img + p * 3;
        const int r = q[0], g = q[1], bl = q[2], L = luma8(r, g, bl);
        q[0] = (unsigned char)blend8(L, r, f);
        q[1] = (unsigned char)blend8(L, g, f);
        q[2] = (unsigned char)blend8(L, bl, f);
      }
      __syncthreads();
    } else if (id == DEVIT_OP_SHARPNESS || id == DEVIT_OP_ROTATE || (id >= DEVIT_OP_SHEAR_X && id <= DEVIT_OP_TRANSLATE_Y)) {
      // neighbour ops: every output pixel of this thread into registers, a barrier, then back into the image
      unsigned stage[OPS_PIX];
#pragma unroll
      for (int j = 0; j < OPS_PIX; ++j) stage[j] = 0;
      int tl = tid;      // opaque per layer: the 98 write-back addresses are otherwise computed once before the layer loop and held in 98 registers
      asm volatile("" : "+v"(tl));
      // A shift register: the newest pixel enters at index 0 and everything moves up one, so every index is static and the array stays in
      // registers (indexed by k it would live in scratch).  Pixels are taken last to first: pixel k ends at stage[k].
#pragma unroll 1
      for (int k = kmax - 1; k >= 0; --k) {
        const unsigned v = neighbour_pixel(min(tl + k * OPS_THREADS, SS - 1), S, op, l);
#pragma unroll
        for (int j = OPS_PIX - 1; j > 0; --j) stage[j] = stage[j - 1];
        stage[0] = v;
      }
      __syncthreads();
#pragma unroll
      for (int j = 0; j < OPS_PIX; ++j) {
        const int p = min(tl + j * OPS_THREADS, SS - 1);      // (threads past the end staged the last pixel's own value: they store it once more)
        if (j < kmax) {
          unsigned char* q = img + p * 3;
          q[0] = (unsigned char)stage[j];
          q[1] = (unsigned char)(stage[j] >> 8);
          q[2] = (unsigned char)(stage[j] >> 16);
        }
      }
      __syncthreads();
    } else if (id >= 0 && id < DEVIT_OP_COUNT) {           // a 3 x 256 table, applied in place
      if (id == DEVIT_OP_AUTOCONTRAST || id == DEVIT_OP_EQUALIZE) {
        for (int i = tid; i < 3 * 256; i += OPS_THREADS) s_hist[i] = 0;
        __syncthreads();
        for (int i = tid; i < n4; i += OPS_THREADS) {
          const unsigned q = img32[i];
          const int c0 = i % 3;                            // channel of byte 4 i
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int c = (c0 + j) % 3;
            atomicAdd(&s_hist[c * 256 + ((q >> (8 * j)) & 255u)], 1);
          }
        }
        __syncthreads();
        if (tid < 3) {
          int* h = s_hist + tid * 256;
          int lo = 256, hi = -1, bins = 0, last = 0, total = 0;
          for (int i = 0; i < 256; ++i) {
            const int n = h[i];
            if (n) {
              if (lo == 256) lo = i;
              hi = i;
              ++bins;
              last = n;
            }
            h[i] = total;
            total += n;
          }
          s_stat[tid * 4 + 0] = lo;
          s_stat[tid * 4 + 1] = hi;
          s_stat[tid * 4 + 2] = bins;
          s_stat[tid * 4 + 3] = (total - last) / 255;
        }
      } else if (id == DEVIT_OP_CONTRAST) {
        if (tid == 0) *s_sum = 0;
        __syncthreads();
        int sum = 0;
        for (int p = tid; p < SS; p += OPS_THREADS) sum += luma8(img[p * 3], img[p * 3 + 1], img[p * 3 + 2]);
        atomicAdd(s_sum, sum);                             // integers: any order gives the same sum
      }
      __syncthreads();
      for (int i = tid; i < 3 * 256; i += OPS_THREADS) {
        const int c = i >> 8, u = i & 255;
        int v = u;
        if (id == DEVIT_OP_AUTOCONTRAST) {
#pragma clang fp contract(off)
          const int lo = s_stat[c * 4], hi = s_stat[c * 4 + 1];
          if (hi > lo) {
            const double scale = 255.0 / (double)(hi - lo), off = (double)(-lo) * scale;
            v = clampi((int)((double)u * scale + off), 0, 255);
          }
        } else if (id == DEVIT_OP_EQUALIZE) {
          const int step = s_stat[c * 4 + 3];
          if (s_stat[c * 4 + 2] > 1 && step > 0) v = min(255, (step / 2 + s_hist[c * 256 + u]) / step);
        } else if (id == DEVIT_OP_INVERT) {
          v = 255 - u;
        } else if (id == DEVIT_OP_POSTERIZE) {
          v = u & ~((1 << (8 - clampi(arg, 0, 8))) - 1);
        } else if (id == DEVIT_OP_SOLARIZE) {
          v = u < arg ? u : 255 - u;
        } else if (id == DEVIT_OP_SOLARIZE_ADD) {
          v = u < 128 ? min(255, u + clampi(arg, 0, 255)) : u;
        } else if (id == DEVIT_OP_BRIGHTNESS) {
          v = blend8(0, u, f);
        } else {                                           // DEVIT_OP_CONTRAST
#pragma clang fp contract(off)
          v = blend8(clampi((int)((double)*s_sum / (double)SS + 0.5), 0, 255), u, f);
        }
        s_lut[i] = (unsigned char)v;
      }
      __syncthreads();
      for (int i = tid; i < n4; i += OPS_THREADS) {
        const unsigned q = img32[i];
        const int c0 = i % 3;
        unsigned o = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) o |= (unsigned)s_lut[((c0 + j) % 3) * 256 + ((q >> (8 * j)) & 255u)] << (8 * j);
        img32[i] = o;
      }
      __syncthreads();
    }
  }

  if constexpr (!FINISH) {
    unsigned* g = (unsigned*)(out8 + (size_t)b * SS * 3);
    for (int i = tid; i < n4; i += OPS_THREADS) g[i] = img32[i];
  } else {
    const devit_augment_sample* sp = table + b;
    const int n_erase = clampi(sp->n_erase, 0, DEVIT_AUGMENT_MAX_ERASE), erase_mode = sp->erase_mode;
    const unsigned long long N = sp->noise_base + (unsigned long long)b;
    if (erase_mode == DEVIT_AUG_ERASE_RAND && tid < n_erase * 3) {
      const int e = tid / 3, c = tid % 3;
      s_rand[e * 3 + c] = normals4(noise_words(N, c, 0x80000000u + (unsigned)e, k0, k1))[0];
    }
    for (int i = tid; i < 3 * 256; i += OPS_THREADS) {
      const int c = i >> 8;
      s_norm[i] = ((float)(i & 255) / 255.0f - norm.mean[c]) / norm.std[c];
    }
    __syncthreads();
    const int nq = S >> 2, items = 3 * S * nq;
    for (int t = tid; t < items; t += OPS_THREADS) {
      const int xq = t % nq, rest = t / nq, yy = rest % S, c = rest / S, x = xq * 4;
      const unsigned char* q = img + (yy * S + x) * 3 + c;
      f32x4 v;
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = s_norm[c * 256 + q[3 * j]];
      unsigned inside = 0;      // bit 4 e + j: pixel j lies in box e
      for (int eb = 0; eb < n_erase; ++eb) {
        const int top = sp->erase[eb][0], left = sp->erase[eb][1], eh = sp->erase[eb][2], ew = sp->erase[eb][3];
        if (yy >= top && yy - top < eh) {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (x + j >= left && x + j - left < ew) inside |= 1u << (4 * eb + j);
        }
      }
      if (inside) {
        f32x4 z = {0.f, 0.f, 0.f, 0.f};
        if (erase_mode == DEVIT_AUG_ERASE_PIXEL) z = normals4(noise_words(N, c, (unsigned)(yy * S + x) >> 2, k0, k1));
#pragma unroll
        for (int eb = 0; eb < DEVIT_AUGMENT_MAX_ERASE; ++eb) {      // later boxes win
          const float zr = erase_mode == DEVIT_AUG_ERASE_RAND ? s_rand[eb * 3 + c] : 0.f;
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (inside >> (4 * eb + j) & 1u) v[j] = erase_mode == DEVIT_AUG_ERASE_PIXEL ? z[j] : zr;
        }
      }
      store16_stream(out + (((size_t)b * 3 + c) * S + yy) * S + x, v);
    }
  }
}

template <bool FINISH>
int launch_image_ops(const char* who, const unsigned char* in, const devit_augment_ops* ops, int B, int S, unsigned char* out8,
                     const devit_augment_sample* table, Norm3 norm, unsigned long long seed, float* out, void* stream) {
  static bool attr_set = false;
  if (!attr_set) {
    hipError_t e = hipFuncSetAttribute((const void*)image_ops_kernel<FINISH>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       224 * 224 * 3 + OPS_FIXED_LDS);
    DEVIT_CHECK(e == hipSuccess, DEVIT_ERR_LAUNCH, "%s: hipFuncSetAttribute: %s", who, hipGetErrorString(e));
    attr_set = true;
  }
  hipLaunchKernelGGL(image_ops_kernel<FINISH>, dim3(B), dim3(OPS_THREADS), S * S * 3 + OPS_FIXED_LDS, (hipStream_t)stream, in, ops, S, out8,
                     table, norm, (unsigned)(seed & 0xffffffffull), (unsigned)(seed >> 32), out);
  DEVIT_LAUNCH_CHECK();
  return DEVIT_OK;
}

int check_geometry(const char* who, int B, int S) {
  DEVIT_CHECK(B > 0 && B <= 65535, DEVIT_ERR_ARG, "%s: B = %d, 1 .. 65535 samples per call", who, B);
  DEVIT_CHECK(devit_patch_grid(3, S, S, 16) != 0, DEVIT_ERR_SHAPE, "%s: output side %d: " DEVIT_PATCH_SIZES_MSG, who, S);
  return DEVIT_OK;
}

// ---- packed sets of mixed image sizes (include/devit_hip.h, "Packed sets"): the image's base, H0 and W0 come from a directory entry --------
constexpr int TAPS_MAX = DEVIT_AUGMENT_TAPS_MAX;
constexpr int WBAND = 16;             // output rows per workgroup of the wide kernel: their accumulators are 48 registers of thread x

// The closed-form bound on the taps an axis needs (the header states it): never below the exact count, so a sample it calls narrow is narrow.
__device__ __forceinline__ int axis_taps(int len, int R, int filter) {
#pragma clang fp contract(off)
  if ((filter != DEVIT_AUG_BILINEAR && filter != DEVIT_AUG_BICUBIC) || len <= 0 || R <= 0) return 1;
  const double scale = (double)len / (double)R;
  const double support = (filter == DEVIT_AUG_BICUBIC ? 2.0 : 1.0) * (scale < 1.0 ? 1.0 : scale);
  const double nd = floor(2.0 * support) + 1.0;
  return nd >= (double)len ? len : (int)nd;
}
__device__ __forceinline__ bool sample_is_wide(const devit_augment_sample* s) {
  return max(axis_taps(s->h, s->Rh, s->filter), axis_taps(s->w, s->Rw, s->filter)) > TAPS;
}

struct RaggedImage {
  const unsigned char* base;
  int H0, W0;
  bool ok;      // false: the entry reaches outside the arena; every pixel then reads 0 (from the arena's first bytes, masked)
};
__device__ __forceinline__ RaggedImage ragged_image(const unsigned char* arena, size_t arena_bytes, const devit_image_entry* entries, int n_img,
                                                    int i) {
  const devit_image_entry e = entries[clampi(i, 0, n_img - 1)];
  const bool dims = e.H >= 1 && e.W >= 1;
  const unsigned long long extent = dims ? 3ull * (unsigned long long)e.H * (unsigned long long)e.W : 0ull;      // < 2^64 for 31-bit sides
  const bool ok = dims && e.offset <= arena_bytes && extent <= arena_bytes - e.offset;
  return RaggedImage{ok ? arena + e.offset : arena, ok ? e.H : 1, ok ? e.W : 1, ok};
}

// PIL's coefficients for T planes of weights: resample_coeffs' operations in its order (the same bits for counts up to TAPS), the weights
// computed twice instead of held, since T of them do not fit registers
__global__ __launch_bounds__(256) void ragged_coeffs_kernel(const devit_augment_sample* __restrict__ table, int B, int S, int T,
                                                            int* __restrict__ ws) {
#pragma clang fp contract(off)
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= B * 2 * S) return;
  const int j = t % S, axis = (t / S) & 1, b = t / (2 * S);
  const devit_augment_sample* s = table + b;
  const int len = axis ? s->w : s->h, R = axis ? s->Rw : s->Rh, xx = (axis ? s->ox : s->oy) + j, filter = s->filter;
  int* p = ws + (size_t)(b * 2 + axis) * (2 + T) * S + j;
  if (!((filter == DEVIT_AUG_BILINEAR || filter == DEVIT_AUG_BICUBIC) && len > 0 && R > 0)) {      // unit scale: the pixel itself
    p[0] = xx;
    p[S] = 1;
    for (int k = 0; k < T; ++k) p[(size_t)(2 + k) * S] = k == 0 ? WEIGHT_ONE : 0;
    return;
  }
  const int cubic = filter == DEVIT_AUG_BICUBIC;
  const double scale = (double)len / (double)R;
  const double fs = scale < 1.0 ? 1.0 : scale;
  const double support = (cubic ? 2.0 : 1.0) * fs;
  const double center = (xx + 0.5) * scale;
  const double ss = 1.0 / fs;
  int xmin = (int)(center - support + 0.5);
  if (xmin < 0) xmin = 0;
  if (xmin > len) xmin = len;
  int xmax = (int)(center + support + 0.5);
  if (xmax > len) xmax = len;
  int n = xmax - xmin;
  n = n < 0 ? 0 : (n > T ? T : n);
  double ww = 0.0;
  for (int k = 0; k < n; ++k) ww += filter_weight((k + xmin - center + 0.5) * ss, cubic);
  p[0] = xmin;
  p[S] = n;
  for (int k = 0; k < T; ++k) {
    double v = 0.0;
    if (k < n) {
      v = filter_weight((k + xmin - center + 0.5) * ss, cubic);
      if (ww != 0.0) v /= ww;
    }
    p[(size_t)(2 + k) * S] = v < 0 ? (int)(-0.5 + v * (double)WEIGHT_ONE) : (int)(0.5 + v * (double)WEIGHT_ONE);
  }
}

// what a ragged kernel needs of steps 3 and 4 (staged by stage_finish, read by finish_quad)
struct FinishLds {
  float rand[DEVIT_AUGMENT_MAX_ERASE][3];
  float norm[3][256];
};
__device__ __forceinline__ void stage_finish(FinishLds& f, const devit_augment_sample* sp, int b, int tid, const Norm3& norm, unsigned k0, unsigned k1) {
  const int n_erase = clampi(sp->n_erase, 0, DEVIT_AUGMENT_MAX_ERASE);
  const unsigned long long N = sp->noise_base + (unsigned long long)b;
  if (sp->erase_mode == DEVIT_AUG_ERASE_RAND && tid < n_erase * 3) {
    const int e = tid / 3, c = tid % 3;
    f.rand[e][c] = normals4(noise_words(N, c, 0x80000000u + (unsigned)e, k0, k1))[0];
  }
  for (int i = tid; i < 3 * 256; i += THREADS) {
    const int c = i >> 8;
    f.norm[c][i & 255] = ((float)(i & 255) / 255.0f - norm.mean[c]) / norm.std[c];
  }
}
// steps 3 and 4 on output pixels (yy, x .. x + 3) of channel c, u their levels after the flip: augment_kernel's statements
__device__ __forceinline__ void finish_quad(const FinishLds& f, const devit_augment_sample* sp, int b, int c, int yy, int x, int S,
                                            const int (&u)[4], unsigned k0, unsigned k1, float* __restrict__ out) {
  const int n_erase = clampi(sp->n_erase, 0, DEVIT_AUGMENT_MAX_ERASE), erase_mode = sp->erase_mode;
  const unsigned long long N = sp->noise_base + (unsigned long long)b;
  f32x4 v;
#pragma unroll
  for (int j = 0; j < 4; ++j) v[j] = f.norm[c][u[j]];
  unsigned inside = 0;      // bit 4 e + j: pixel j lies in box e
  for (int eb = 0; eb < n_erase; ++eb) {
    const int top = sp->erase[eb][0], left = sp->erase[eb][1], eh = sp->erase[eb][2], ew = sp->erase[eb][3];
    if (yy >= top && yy - top < eh) {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (x + j >= left && x + j - left < ew) inside |= 1u << (4 * eb + j);
    }
  }
  if (inside) {
    f32x4 z = {0.f, 0.f, 0.f, 0.f};
    if (erase_mode == DEVIT_AUG_ERASE_PIXEL) z = normals4(noise_words(N, c, (unsigned)(yy * S + x) >> 2, k0, k1));
#pragma unroll
    for (int eb = 0; eb < DEVIT_AUGMENT_MAX_ERASE; ++eb) {      // later boxes win
      const float zr = erase_mode == DEVIT_AUG_ERASE_RAND ? f.rand[eb][c] : 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (inside >> (4 * eb + j) & 1u) v[j] = erase_mode == DEVIT_AUG_ERASE_PIXEL ? z[j] : zr;
    }
  }
  store16_stream(out + (((size_t)b * 3 + c) * S + yy) * S + x, v);
}

// The narrow kernel: augment_kernel (U8: augment_u8_kernel) with the image taken from the directory.  Samples the closed form calls wide are
// the wide kernel's when it runs (wide_on): their workgroups leave at once.  The workspace has T weight planes; this kernel reads the first TAPS.
template <bool U8>
__global__ __launch_bounds__(THREADS) void ragged_narrow_kernel(const unsigned char* __restrict__ arena, size_t arena_bytes,
                                                                const devit_image_entry* __restrict__ entries, int n_img,
                                                                const int* __restrict__ idx, const devit_augment_sample* __restrict__ table,
                                                                int S, int T, const int* __restrict__ ws, int wide_on, Norm3 norm, unsigned k0,
                                                                unsigned k1, float* __restrict__ out, unsigned char* __restrict__ out8) {
  __shared__ __attribute__((aligned(16))) unsigned char inter[3][NROWS][PITCH];
  __shared__ int s_ymin[BAND], s_yn[BAND], s_wy[BAND][TAPS];
  __shared__ FinishLds fin;
  const int tid = threadIdx.x, b = blockIdx.y, r0 = blockIdx.x * BAND, r1 = min(r0 + BAND, S);
  const devit_augment_sample* sp = table + b;
  if (wide_on && sample_is_wide(sp)) return;      // the same for every thread of the workgroup
  const int y0 = sp->y0, x0 = sp->x0, flip = sp->flip;
  const RaggedImage im = ragged_image(arena, arena_bytes, entries, n_img, idx[b]);
  const unsigned char* image = im.base;
  const int H0 = im.H0, W0 = im.W0, planes = 2 + T;
  const int* wsy = ws + (size_t)(b * 2) * planes * S;
  const int* wsx = wsy + (size_t)planes * S;

  // the band's vertical coefficients -> LDS; column tid's horizontal ones -> registers
  for (int i = tid; i < BAND * PLANES; i += THREADS) {
    const int r = i / PLANES, q = i % PLANES;
    const int v = wsy[(size_t)min(q, planes - 1) * S + min(r0 + r, S - 1)];
    if (q == 0) s_ymin[r] = v;
    else if (q == 1) s_yn[r] = clampi(v, 0, min(T, TAPS));
    else s_wy[r][q - 2] = q < planes ? v : 0;
  }
  const int xc = min(tid, S - 1);
  const int xmin_x = wsx[xc];
  int wx[TAPS];
#pragma unroll
  for (int k = 0; k < TAPS; ++k) {
    const int v = wsx[(size_t)min(2 + k, planes - 1) * S + xc];
    wx[k] = k < T ? v : 0;
  }
  if constexpr (!U8) stage_finish(fin, sp, b, tid, norm, k0, k1);

  // vertical pass: a wave takes 64 / nq (row, channel) pairs at a time, lane -> (pair, quad of four output pixels)
  const int nq = S >> 2, lane = tid & 63, per = 64 / nq, sub = lane / nq, xq = lane - sub * nq;
  const int x = xq * 4, xs = flip ? S - 4 - x : x;
  int r = r0;
  while (r < r1) {
    __syncthreads();      // the coefficients are staged; the previous run's intermediate has been read
    const int lo = s_ymin[r - r0];
    int e = r + 1;        // one output row needs at most TAPS <= NROWS source rows: every run advances
    while (e < r1 && s_ymin[e - r0] + s_yn[e - r0] - lo <= NROWS) ++e;
    const int nrows = clampi(s_ymin[e - 1 - r0] + s_yn[e - 1 - r0] - lo, 0, NROWS);

    // horizontal pass: source rows lo .. lo + nrows of the box, output column tid
    if (tid < S) {
      for (int row = 0; row < nrows; ++row) {
        const int sy = y0 + lo + row;
        const bool in_y = im.ok && sy >= 0 && sy < H0;
        const unsigned char* line = image + (size_t)clampi(sy, 0, H0 - 1) * W0 * 3;
        int a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21;
#pragma unroll
        for (int k = 0; k < TAPS; ++k) {
          const int sx = x0 + xmin_x + k;
          const bool ok = in_y && sx >= 0 && sx < W0;
          const unsigned char* p = line + (size_t)clampi(sx, 0, W0 - 1) * 3;
          const int p0 = p[0], p1 = p[1], p2 = p[2];
          const int w = ok ? wx[k] : 0;
          a0 += p0 * w;
          a1 += p1 * w;
          a2 += p2 * w;
        }
        inter[0][row][tid] = (unsigned char)clampi(a0 >> 22, 0, 255);
        inter[1][row][tid] = (unsigned char)clampi(a1 >> 22, 0, 255);
        inter[2][row][tid] = (unsigned char)clampi(a2 >> 22, 0, 255);
      }
    }
    __syncthreads();

    // vertical pass, flip, then steps 3 and 4 or the uint8 window: four output pixels of one row and channel per item
    const int pairs = (e - r) * 3;
    for (int t = (tid >> 6) * per + sub; sub < per && t < pairs; t += (THREADS / 64) * per) {
      const int c = t % 3, yy = r + t / 3;
      const int ymin = s_ymin[yy - r0] - lo, yn = s_yn[yy - r0];
      int acc[4] = {1 << 21, 1 << 21, 1 << 21, 1 << 21};
      for (int k = 0; k < yn; ++k) {
        const unsigned q = *(const unsigned*)&inter[c][clampi(ymin + k, 0, NROWS - 1)][xs];
        const int w = s_wy[yy - r0][k];
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] += (int)((q >> (8 * j)) & 255u) * w;
      }
      int u[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) u[j] = clampi((flip ? acc[3 - j] : acc[j]) >> 22, 0, 255);
      if constexpr (U8) {
#pragma unroll
        for (int j = 0; j < 4; ++j) out8[(((size_t)b * S + yy) * S + x + j) * 3 + c] = (unsigned char)u[j];
      } else {
        finish_quad(fin, sp, b, c, yy, x, S, u, k0, k1, out);
      }
    }
    r = e;
  }
}

// The wide kernel: up to TAPS_MAX taps per axis.  One workgroup per (sample, band of WBAND output rows); thread x owns output column x.  It walks
// the band's source rows once: the row's horizontal result for its column (weights read [k][x] from the workspace, clamped to uint8 as PIL's
// intermediate is), added at once, weighted, into the accumulators of the output rows whose vertical window holds that source row.  No
// intermediate image, so no limit on the rows a band spans.  The finished rows go through LDS to the quad-wise finish of the narrow kernel.
template <bool U8>
__global__ __launch_bounds__(THREADS) void ragged_wide_kernel(const unsigned char* __restrict__ arena, size_t arena_bytes,
                                                              const devit_image_entry* __restrict__ entries, int n_img,
                                                              const int* __restrict__ idx, const devit_augment_sample* __restrict__ table,
                                                              int S, int T, const int* __restrict__ ws, int force, Norm3 norm, unsigned k0,
                                                              unsigned k1, float* __restrict__ out, unsigned char* __restrict__ out8) {
  __shared__ __attribute__((aligned(16))) unsigned char tile[3][WBAND][PITCH];
  __shared__ int s_ymin[WBAND], s_yn[WBAND], s_wy[WBAND][TAPS_MAX];
  __shared__ FinishLds fin;
  const int tid = threadIdx.x, b = blockIdx.y, r0 = blockIdx.x * WBAND, nb = min(WBAND, S - r0);
  const devit_augment_sample* sp = table + b;
  if (!force && !sample_is_wide(sp)) return;      // the same for every thread of the workgroup
  const int y0 = sp->y0, x0 = sp->x0, flip = sp->flip;
  const RaggedImage im = ragged_image(arena, arena_bytes, entries, n_img, idx[b]);
  const int H0 = im.H0, W0 = im.W0, planes = 2 + T;
  const int* wsy = ws + (size_t)(b * 2) * planes * S;
  const int* wsx = wsy + (size_t)planes * S;

  for (int i = tid; i < WBAND * planes; i += THREADS) {
    const int r = i / planes, q = i - r * planes;
    const int v = wsy[(size_t)q * S + min(r0 + r, S - 1)];
    if (q == 0) s_ymin[r] = v;
    else if (q == 1) s_yn[r] = r < nb ? clampi(v, 0, T) : 0;
    else s_wy[r][q - 2] = v;
  }
  const int xc = min(tid, S - 1);
  const int xmin_x = wsx[xc], nx = clampi(wsx[S + xc], 0, T);
  const int* wcol = wsx + (size_t)2 * S + xc;
  if constexpr (!U8) stage_finish(fin, sp, b, tid, norm, k0, k1);
  __syncthreads();

  int ym[WBAND], yn[WBAND], acc[WBAND][3];      // (uniform values: scalar registers)
#pragma unroll
  for (int r = 0; r < WBAND; ++r) {
    ym[r] = __builtin_amdgcn_readfirstlane(s_ymin[r]);
    yn[r] = __builtin_amdgcn_readfirstlane(s_yn[r]);
    acc[r][0] = acc[r][1] = acc[r][2] = 1 << 21;
  }
  // the rows' windows abut or overlap (the centres advance by the scale, a window is at least twice that): their union is one run of at most
  // WBAND * T source rows
  const int lo = ym[0];
  const int nrows = clampi(__builtin_amdgcn_readfirstlane(s_ymin[nb - 1] + s_yn[nb - 1]) - lo, 0, WBAND * TAPS_MAX);
  if (tid < S) {
    for (int row = 0; row < nrows; ++row) {
      const int sy = y0 + lo + row;
      const bool in_y = im.ok && sy >= 0 && sy < H0;
      const unsigned char* line = im.base + (size_t)clampi(sy, 0, H0 - 1) * W0 * 3;
      int a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21;
      for (int k = 0; k < nx; ++k) {
        const int sx = x0 + xmin_x + k;
        const bool ok = in_y && sx >= 0 && sx < W0;
        const unsigned char* p = line + (size_t)clampi(sx, 0, W0 - 1) * 3;
        const int p0 = p[0], p1 = p[1], p2 = p[2];
        const int w = ok ? wcol[(size_t)k * S] : 0;
        a0 += p0 * w;
        a1 += p1 * w;
        a2 += p2 * w;
      }
      const int h0 = clampi(a0 >> 22, 0, 255), h1 = clampi(a1 >> 22, 0, 255), h2 = clampi(a2 >> 22, 0, 255);      // PIL's uint8 intermediate
#pragma unroll
      for (int r = 0; r < WBAND; ++r) {
        const int k = lo + row - ym[r];
        if (k >= 0 && k < yn[r]) {
          const int w = s_wy[r][k];
          acc[r][0] += h0 * w;
          acc[r][1] += h1 * w;
          acc[r][2] += h2 * w;
        }
      }
    }
#pragma unroll
    for (int r = 0; r < WBAND; ++r) {
#pragma unroll
      for (int c = 0; c < 3; ++c) tile[c][r][tid] = (unsigned char)clampi(acc[r][c] >> 22, 0, 255);
    }
  }
  __syncthreads();

  const int nq = S >> 2, lane = tid & 63, per = 64 / nq, sub = lane / nq, xq = lane - sub * nq;
  const int x = xq * 4, xs = flip ? S - 4 - x : x;
  for (int t = (tid >> 6) * per + sub; sub < per && t < nb * 3; t += (THREADS / 64) * per) {
    const int c = t % 3, rr = t / 3, yy = r0 + rr;
    const unsigned q = *(const unsigned*)&tile[c][rr][xs];
    int u[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) u[j] = (int)((q >> (8 * (flip ? 3 - j : j))) & 255u);
    if constexpr (U8) {
#pragma unroll
      for (int j = 0; j < 4; ++j) out8[(((size_t)b * S + yy) * S + x + j) * 3 + c] = (unsigned char)u[j];
    } else {
      finish_quad(fin, sp, b, c, yy, x, S, u, k0, k1, out);
    }
  }
}

template <bool U8>
void launch_ragged(const unsigned char* arena, size_t arena_bytes, const devit_image_entry* entries, int n, const int* idx,
                   const devit_augment_sample* table, int B, int S, int T, const int* ws, unsigned flags, Norm3 norm, unsigned long long seed,
                   float* out, unsigned char* out8, hipStream_t stream) {
  const int force = (flags & DEVIT_AUGMENT_FORCE_WIDE) != 0, wide_on = force || T > TAPS;
  const unsigned k0 = (unsigned)(seed & 0xffffffffull), k1 = (unsigned)(seed >> 32);
  if (!force)
    hipLaunchKernelGGL(ragged_narrow_kernel<U8>, dim3((S + BAND - 1) / BAND, B), dim3(THREADS), 0, stream, arena, arena_bytes, entries, n, idx,
                       table, S, T, ws, wide_on, norm, k0, k1, out, out8);
  if (wide_on)
    hipLaunchKernelGGL(ragged_wide_kernel<U8>, dim3((S + WBAND - 1) / WBAND, B), dim3(THREADS), 0, stream, arena, arena_bytes, entries, n, idx,
                       table, S, T, ws, force, norm, k0, k1, out, out8);
}

}  // namespace

extern "C" size_t devit_augment_workspace(int B, int S) {
  if (B <= 0 || S <= 0) return 0;
  return (size_t)B * 2 * PLANES * S * sizeof(int);
}

extern "C" int devit_augment_coeffs(const devit_augment_sample* table, int B, int S, void* workspace, size_t workspace_bytes,
                                    void* stream) {
  if (int rc = check_geometry("devit_augment_coeffs", B, S)) return rc;
  DEVIT_CHECK(table && workspace && workspace_bytes >= devit_augment_workspace(B, S), DEVIT_ERR_ARG,
              "devit_augment_coeffs: null pointer or a workspace below devit_augment_workspace(B, S)");
  hipLaunchKernelGGL(augment_coeffs_kernel, dim3((B * 2 * S + 255) / 256), dim3(256), 0, (hipStream_t)stream, table, B, S,
                     (int*)workspace);
  DEVIT_LAUNCH_CHECK();
  return DEVIT_OK;
}

extern "C" int devit_augment_batch(const unsigned char* src, int n, int H0, int W0, const int* idx, const devit_augment_sample* table,
                                   int B, int S, const float* mean, const float* std, unsigned long long seed, float* out,
                                   void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = check_geometry("devit_augment_batch", B, S)) return rc;
  DEVIT_CHECK(src && idx && table && mean && std && out && workspace, DEVIT_ERR_ARG, "devit_augment_batch: null pointer");
  DEVIT_CHECK(n > 0 && H0 > 0 && W0 > 0 && H0 <= 4096 && W0 <= 4096, DEVIT_ERR_ARG,
              "devit_augment_batch: a set of %d images of %d x %d (sides 1 .. 4096)", n, H0, W0);
  DEVIT_CHECK(((uintptr_t)out & 15) == 0, DEVIT_ERR_ARG, "devit_augment_batch: out must be 16-byte aligned");
  DEVIT_CHECK(workspace_bytes >= devit_augment_workspace(B, S), DEVIT_ERR_ARG,
              "devit_augment_batch: the workspace holds %zu bytes, devit_augment_workspace(B, S) is %zu", workspace_bytes,
              devit_augment_workspace(B, S));
  Norm3 norm;
  for (int c = 0; c < 3; ++c) {
    DEVIT_CHECK(std[c] > 0.f, DEVIT_ERR_ARG, "devit_augment_batch: std[%d] = %g must be positive", c, (double)std[c]);
    norm.mean[c] = mean[c];
    norm.std[c] = std[c];
  }
  if (int rc = devit_augment_coeffs(table, B, S, workspace, workspace_bytes, stream)) return rc;
  hipLaunchKernelGGL(augment_kernel, dim3((S + BAND - 1) / BAND, B), dim3(THREADS), 0, (hipStream_t)stream, src, n, H0, W0, idx, table,
                     S, (const int*)workspace, norm, (unsigned)(seed & 0xffffffffull), (unsigned)(seed >> 32), out);
  DEVIT_LAUNCH_CHECK();
  return DEVIT_OK;
}

extern "C" int devit_image_ops(const unsigned char* in, const devit_augment_ops* ops, int B, int S, unsigned char* out, void* stream) {
  if (int rc = check_geometry("devit_image_ops", B, S)) return rc;
  DEVIT_CHECK(in && ops && out, DEVIT_ERR_ARG, "devit_image_ops: null pointer");
  DEVIT_CHECK((((uintptr_t)in | (uintptr_t)out) & 3) == 0, DEVIT_ERR_ARG, "devit_image_ops: in and out must be 4-byte aligned");
  return launch_image_ops<false>("devit_image_ops", in, ops, B, S, out, nullptr, Norm3{}, 0ull, nullptr, stream);
}

extern "C" size_t devit_augment_ops_workspace(int B, int S) {
  if (B <= 0 || S <= 0) return 0;
  return ((devit_augment_workspace(B, S) + 15) & ~(size_t)15) + (size_t)B * S * S * 3;
}

extern "C" int devit_augment_batch_ops(const unsigned char* src, int n, int H0, int W0, const int* idx, const devit_augment_sample* table,
                                       const devit_augment_ops* ops, int B, int S, const float* mean, const float* std,
                                       unsigned long long seed, float* out, void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = check_geometry("devit_augment_batch_ops", B, S)) return rc;
  DEVIT_CHECK(src && idx && table && ops && mean && std && out && workspace, DEVIT_ERR_ARG, "devit_augment_batch_ops: null pointer");
  DEVIT_CHECK(n > 0 && H0 > 0 && W0 > 0 && H0 <= 4096 && W0 <= 4096, DEVIT_ERR_ARG,
              "devit_augment_batch_ops: a set of %d images of %d x %d (sides 1 .. 4096)", n, H0, W0);
  DEVIT_CHECK((((uintptr_t)out | (uintptr_t)workspace) & 15) == 0, DEVIT_ERR_ARG,
              "devit_augment_batch_ops: out and the workspace must be 16-byte aligned");
  DEVIT_CHECK(workspace_bytes >= devit_augment_ops_workspace(B, S), DEVIT_ERR_ARG,
              "devit_augment_batch_ops: the workspace holds %zu bytes, devit_augment_ops_workspace(B, S) is %zu", workspace_bytes,
              devit_augment_ops_workspace(B, S));
  Norm3 norm;
  for (int c = 0; c < 3; ++c) {
    DEVIT_CHECK(std[c] > 0.f, DEVIT_ERR_ARG, "devit_augment_batch_ops: std[%d] = %g must be positive", c, (double)std[c]);
    norm.mean[c] = mean[c];
    norm.std[c] = std[c];
  }
  unsigned char* window = (unsigned char*)workspace + ((devit_augment_workspace(B, S) + 15) & ~(size_t)15);
  if (int rc = devit_augment_coeffs(table, B, S, workspace, workspace_bytes, stream)) return rc;
  hipLaunchKernelGGL(augment_u8_kernel, dim3((S + BAND - 1) / BAND, B), dim3(THREADS), 0, (hipStream_t)stream, src, n, H0, W0, idx, table, S,
                     (const int*)workspace, window);
  DEVIT_LAUNCH_CHECK();
  return launch_image_ops<true>("devit_augment_batch_ops", window, ops, B, S, nullptr, table, norm, seed, out, stream);
}

extern "C" size_t devit_augment_ragged_workspace(int B, int S, int max_taps, int with_ops) {
  if (B <= 0 || S <= 0 || max_taps < 1 || max_taps > TAPS_MAX) return 0;
  const size_t coeffs = (size_t)B * 2 * (2 + max_taps) * S * sizeof(int);
  return with_ops ? ((coeffs + 15) & ~(size_t)15) + (size_t)B * S * S * 3 : coeffs;
}

extern "C" int devit_augment_ragged(const unsigned char* arena, size_t arena_bytes, const devit_image_entry* entries, int n, const int* idx,
                                    const devit_augment_sample* table, const devit_augment_ops* ops, int B, int S, const float* mean,
                                    const float* std, unsigned long long seed, float* out, void* workspace, size_t workspace_bytes,
                                    int max_taps, unsigned flags, void* stream) {
  if (int rc = check_geometry("devit_augment_ragged", B, S)) return rc;
  DEVIT_CHECK(arena && entries && idx && table && mean && std && out && workspace, DEVIT_ERR_ARG, "devit_augment_ragged: null pointer");
  DEVIT_CHECK(n > 0 && arena_bytes >= 3, DEVIT_ERR_ARG, "devit_augment_ragged: a set of %d images in an arena of %zu bytes", n, arena_bytes);
  DEVIT_CHECK(max_taps >= 1 && max_taps <= TAPS_MAX, DEVIT_ERR_ARG, "devit_augment_ragged: max_taps = %d, 1 .. %d", max_taps, TAPS_MAX);
  DEVIT_CHECK((flags & ~DEVIT_AUGMENT_FORCE_WIDE) == 0, DEVIT_ERR_ARG, "devit_augment_ragged: unknown flags 0x%x", flags);
  DEVIT_CHECK((((uintptr_t)out | (uintptr_t)workspace) & 15) == 0 && ((uintptr_t)entries & 7) == 0, DEVIT_ERR_ARG,
              "devit_augment_ragged: out and the workspace must be 16-byte aligned, the directory 8-byte aligned");
  const size_t need = devit_augment_ragged_workspace(B, S, max_taps, ops != nullptr);
  DEVIT_CHECK(workspace_bytes >= need, DEVIT_ERR_ARG,
              "devit_augment_ragged: the workspace holds %zu bytes, devit_augment_ragged_workspace(B, S, max_taps, with_ops) is %zu",
              workspace_bytes, need);
  Norm3 norm;
  for (int c = 0; c < 3; ++c) {
    DEVIT_CHECK(std[c] > 0.f, DEVIT_ERR_ARG, "devit_augment_ragged: std[%d] = %g must be positive", c, (double)std[c]);
    norm.mean[c] = mean[c];
    norm.std[c] = std[c];
  }
  hipLaunchKernelGGL(ragged_coeffs_kernel, dim3((B * 2 * S + 255) / 256), dim3(256), 0, (hipStream_t)stream, table, B, S, max_taps,
                     (int*)workspace);
  DEVIT_LAUNCH_CHECK();
  if (!ops) {
    launch_ragged<false>(arena, arena_bytes, entries, n, idx, table, B, S, max_taps, (const int*)workspace, flags, norm, seed, out, nullptr,
                         (hipStream_t)stream);
    DEVIT_LAUNCH_CHECK();
    return DEVIT_OK;
  }
  unsigned char* window = (unsigned char*)workspace + ((devit_augment_ragged_workspace(B, S, max_taps, 0) + 15) & ~(size_t)15);
  launch_ragged<true>(arena, arena_bytes, entries, n, idx, table, B, S, max_taps, (const int*)workspace, flags, norm, seed, nullptr, window,
                      (hipStream_t)stream);
  DEVIT_LAUNCH_CHECK();
  return launch_image_ops<true>("devit_augment_ragged", window, ops, B, S, nullptr, table, norm, seed, out, stream);
}
