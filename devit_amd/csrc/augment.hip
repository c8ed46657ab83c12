// Input augmentation (include/devit_hip.h, "Input augmentation"): a resident uint8 image set -> the normalized fp32 batch.
//   augment_coeffs_kernel   PIL's resampling coefficients per (sample, axis, output index), in IEEE double with contraction off,
//                           as int32 into a workspace: [B][2 axes][2 + TAPS][S] = xmin, count, weights (zero behind the count)
//   augment_kernel          one workgroup per (sample, band of 32 output rows): horizontal pass of the source rows the band needs into
//                           LDS as the uint8 intermediate (thread x keeps column x's taps in registers), then the vertical pass, flip,
//                           normalize (a table of the 256 levels per channel, made with the header's two divisions) and erasing out of
//                           LDS into 16-byte stores.  Integer arithmetic up to the normalization.
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

int check_geometry(const char* who, int B, int S) {
  DEVIT_CHECK(B > 0 && B <= 65535, DEVIT_ERR_ARG, "%s: B = %d, 1 .. 65535 samples per call", who, B);
  DEVIT_CHECK(devit_patch_grid(3, S, S, 16) != 0, DEVIT_ERR_SHAPE, "%s: output side %d: " DEVIT_PATCH_SIZES_MSG, who, S);
  return DEVIT_OK;
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
