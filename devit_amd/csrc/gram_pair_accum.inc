// The Gram accumulation of the Gram-pair tile: defines gram_accumulate<F16>() for the including unit (gram_pair.h explains why a text fragment).
// acc[h][J] += X_ci[strip h of this wave][:] X_cj[tile J][:]^T over the D columns of the image at `img` (row stride ld, N live rows, F16: f16 lanes).
// Wave w owns the 16-row strips w and w + 8 (`two`: the second exists); every strip spans all 13 column tiles, so a row's statistics stay inside one
// wave.  diag (ci == cj): one LDS image, stages 0 / 1 of `lds`, serves the A and the B fragments.  Otherwise stages 0 / 1 hold the A operand's 64-wide
// K chunks and stages 2 / 3 the B operand's; the A chunk's successor travels through registers under the MFMAs, the B chunk's is fetched behind them
// (one set of prefetch registers beside 2 x 2 x 13 accumulators).  Rows >= N are never loaded: the LDS image holds zeros there.  Ends behind a
// barrier: the stages may be rewritten at once.
//   GP_ACCUM_PARAMS                 the unit's own parameters, each followed by a comma
//   GP_ACCUM_SETUP                  statements: `diag`, `ci`, `cj` and the lane values of the loader; ends behind a barrier if it writes LDS
//   GP_ACCUM_LOAD(dst, u, comp, c)  statement: dst = the thread's u-th 16-byte piece (piece tid % 8 of row tid / 8 + 64 u) of chunk c of component
//                                   comp, `zero` for a row that is not loaded
template <bool F16>
__device__ __forceinline__ void gram_accumulate(const __bf16* img, int ld, int D, int N, GP_ACCUM_PARAMS char* lds, int wave, int lane, bool two,
                                                f32x4 (&acc)[2][GP_TILES]) {
  const int tid = threadIdx.x, nch = D / 64;
  const bf16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
  bf16x8 pf[4];
  GP_ACCUM_SETUP
  auto gload = [&](int comp, int c) {
#pragma unroll
    for (int u = 0; u < 4; ++u) GP_ACCUM_LOAD(pf[u], u, comp, c)
  };
  auto lstore = [&](int stage) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int sg = tid + u * 512, row = sg >> 3, piece = sg & 7;
      if (sg < GP_SEGS) *(bf16x8*)(lds + stage * GP_STAGE + row * GP_STRIDE + piece * 16) = pf[u];
    }
  };
  gload(ci, 0);
  lstore(0);
  if (!diag) {
    gload(cj, 0);
    lstore(2);
  }
  __syncthreads();
  const int frag = (lane & 15) * GP_STRIDE + (lane >> 4) * 16;     // row x of a tile, k = 8 g .. 8 g + 7 of a 32-wide step
  for (int c = 0; c < nch; ++c) {
    if (c + 1 < nch) gload(ci, c + 1);
    const char* sa = lds + (c & 1) * GP_STAGE + frag;
    const char* sb = diag ? sa : sa + 2 * GP_STAGE;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      const bf16x8 a0 = *(const bf16x8*)(sa + wave * 16 * GP_STRIDE + kk * 64);
      bf16x8 a1 = zero;
      if (two) a1 = *(const bf16x8*)(sa + (wave + 8) * 16 * GP_STRIDE + kk * 64);
#pragma unroll
      for (int J = 0; J < GP_TILES; ++J) {
        const bf16x8 bj = *(const bf16x8*)(sb + J * 16 * GP_STRIDE + kk * 64);
        acc[0][J] = mfma16t<F16>(a0, bj, acc[0][J]);
        if (two) acc[1][J] = mfma16t<F16>(a1, bj, acc[1][J]);
      }
    }
    if (c + 1 < nch) {
      lstore((c + 1) & 1);
      if (!diag) {
        gload(cj, c + 1);
        lstore(2 + ((c + 1) & 1));
      }
    }
    __syncthreads();
  }
}
