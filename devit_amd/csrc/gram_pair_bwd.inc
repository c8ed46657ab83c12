// The backward of the Gram-pair tile, the body of a __global__ kernel of 512 threads: one workgroup per (image b, component ci).
// d_i^T[c][r] = sum_j sum_k X_j^T[c][k] S_ij[r][k], 64 columns c at a time, NJ = 1 (j = ci, slot ci) or 3 products per chunk (j = 0 .. 2, slots
// 3 ci + j), times the device scalar in fp32 before the one bf16 rounding.  B operand = the image's S, read from HBM once per j into registers (lane
// (n, g): row 16 it + n, k = 32 ks + 8 g .. + 7; wave w owns the row tiles w and w + 8; every element of the slots was written by the forward: all
// 208 rows x 224 columns are read); A operand = X_j^T by transposed reads from the LDS image of the 64-column chunk (as attention reads V).  The
// (chunk, j) steps alternate between two stages of `lds`, the next step's chunk on its way through registers meanwhile.  The launch bounds, the
// upstream index and the row addressing are the including kernel's.
//   reads    : `a` (S, B, N, Ds), int b, ci; constexpr or template int NJ; char lds[2 * GP_BSTAGE]
//   GP_BWD_SETUP                  statements: the lane values of the loader; ends behind a barrier if it writes LDS
//   GP_BWD_LOAD(dst, u, comp, c)  statement: dst = the thread's u-th 16-byte piece (piece tid % 8 of row tid / 8 + 64 u) of chunk c of component
//                                 comp, `zero` for a row that is not loaded
//   GP_BWD_EACH_PRODUCT(j)        the head of the statement that runs the products j = 0 .. NJ - 1 of one chunk
//   GP_BWD_UPSTREAM               the device scalar
//   GP_BWD_OUT(o, i, c)           statement: declares __bf16* o, the first of this lane's columns (4 g ..) of row i's chunk c of d_ci
const int N = a.N, nch = a.Ds / 64, steps = nch * NJ;
const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63, tid = threadIdx.x;
const bool two = wave + 8 < GP_TILES;
const int n = lane & 15, g = lane >> 4;
const bf16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
bf16x8 pf[4];
GP_BWD_SETUP
auto gload = [&](int step) {
  const int c = step / NJ, comp = NJ == 1 ? ci : step - c * NJ;
#pragma unroll
  for (int u = 0; u < 4; ++u) GP_BWD_LOAD(pf[u], u, comp, c)
};
auto lstore = [&](int stage) {
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int sg = tid + u * 512, row = sg >> 3, piece = sg & 7;
    if (sg < GP_BSEGS) *(bf16x8*)(lds + stage * GP_BSTAGE + row * GP_STRIDE + piece * 16) = pf[u];
  }
};
gload(0);
bf16x8 sf[NJ][2][7];
#pragma unroll
for (int j = 0; j < NJ; ++j) {
  const int slot = NJ == 1 ? ci : 3 * ci + j;
  const __bf16* const Sl = a.S + (((size_t)slot * a.B + b) * GP_ROWS + wave * 16 + n) * GP_SLD + g * 8;
#pragma unroll
  for (int ks = 0; ks < 7; ++ks) {
    sf[j][0][ks] = *(const bf16x8*)(Sl + ks * 32);
    sf[j][1][ks] = two ? *(const bf16x8*)(Sl + (size_t)128 * GP_SLD + ks * 32) : zero;
  }
}
lstore(0);
__syncthreads();
const float up = GP_BWD_UPSTREAM;
// transposed read: lane 4 q + p of a 16-lane group addresses row q, columns 4 p .. 4 p + 3 of a 4 x 16 block and receives column (lane & 15)
const int trd = (8 * g + (n >> 2)) * GP_STRIDE + (n & 3) * 8;
for (int c = 0; c < nch; ++c) {
  f32x4 acc[2][4];
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) acc[h][ct] = (f32x4){0.f, 0.f, 0.f, 0.f};
  GP_BWD_EACH_PRODUCT(j) {
    const int step = c * NJ + j;
    if (step + 1 < steps) gload(step + 1);
    const char* const st = lds + (step & 1) * GP_BSTAGE + trd;
#pragma unroll
    for (int ks = 0; ks < 7; ++ks) {
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) {
        const char* p = st + ks * 32 * GP_STRIDE + ct * 32;
        const bf16x8 ff = cat8(lds_tr_read(p), lds_tr_read(p + 4 * GP_STRIDE));
        acc[0][ct] = mfma16(ff, sf[j][0][ks], acc[0][ct]);
        if (two) acc[1][ct] = mfma16(ff, sf[j][1][ks], acc[1][ct]);
      }
    }
    if (j == NJ - 1) {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int i = (wave + 8 * h) * 16 + n;
        if ((h == 0 || two) && i < N) {
          GP_BWD_OUT(o, i, c)
#pragma unroll
          for (int ct = 0; ct < 4; ++ct) {
            const f32x4 v = acc[h][ct];
            *(bf16x4*)(o + ct * 16) = (bf16x4){f2bf(v[0] * up), f2bf(v[1] * up), f2bf(v[2] * up), f2bf(v[3] * up)};
          }
        }
      }
    }
    if (step + 1 < steps) lstore((step + 1) & 1);
    __syncthreads();
  }
}
