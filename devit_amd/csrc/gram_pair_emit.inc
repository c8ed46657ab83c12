// S emission of the Gram-pair tile, a fragment of a forward kernel's body behind gram_pair_stats.inc and a barrier.
// S[i][j] = coef (e^{s - rls_i} + e^{s - cls_j} - e^{t - rlt_i} - e^{t - clt_j}), zero outside N x N (r*: the rows' base-2 log-sum-exps, c*: the
// columns'; for a symmetric Gram they are the same arrays).  The lane holds four consecutive i of one column j: it writes them as one 8-byte store
// into ROW j of the transposed copy (for a symmetric S the matrix itself: the value computed at (i, j) is as good a rounding of S_ji) and, for a
// Gram that is not symmetric, as four 2-byte stores into the rows i of the matrix.  Columns 208 .. 223 of the strips' rows, the K tail of the
// backward product, are zeroed.
//   reads    : f32x4 at[2][GP_TILES], as[2][GP_TILES] as gram_pair_stats.inc left them; int N, wave, n, g; bool two
//   GP_EMIT_RLT, GP_EMIT_RLS, GP_EMIT_CLT, GP_EMIT_CLS   float arrays in LDS, [208]
//   GP_EMIT_COEF                          the factor
//   GP_EMIT_ST                            __bf16*: the image's [208][224] slot of the transposed copy
//   GP_EMIT_BOTH, GP_EMIT_SR              whether the matrix itself is stored too, and its slot
//   GP_EMIT_LANE                          the lane id
//   GP_ONE_ROW                            1: a scheduling barrier behind every column tile, as gram_pair_stats.inc
#pragma unroll
for (int h = 0; h < 2; ++h) {
  if (h == 0 || two) {
    const int i0 = (wave + 8 * h) * 16 + 4 * g;
    float lti[4], lsi[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      lti[r] = GP_EMIT_RLT[i0 + r];
      lsi[r] = GP_EMIT_RLS[i0 + r];
    }
#pragma unroll
    for (int J = 0; J < GP_TILES; ++J) {
      const int j = J * 16 + n;
      const float ltj = GP_EMIT_CLT[j], lsj = GP_EMIT_CLS[j];
      f32x4 v;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float t = at[h][J][r], s = as[h][J][r];
        const float e = (__builtin_amdgcn_exp2f(s - lsi[r]) + __builtin_amdgcn_exp2f(s - lsj) - __builtin_amdgcn_exp2f(t - lti[r]) -
                         __builtin_amdgcn_exp2f(t - ltj)) * GP_EMIT_COEF;
        v[r] = (i0 + r < N && j < N) ? e : 0.f;
      }
      *(bf16x4*)(GP_EMIT_ST + (size_t)j * GP_SLD + i0) = (bf16x4){f2bf(v[0]), f2bf(v[1]), f2bf(v[2]), f2bf(v[3])};
      if (GP_EMIT_BOTH) {
#pragma unroll
        for (int r = 0; r < 4; ++r) GP_EMIT_SR[(size_t)(i0 + r) * GP_SLD + j] = f2bf(v[r]);
      }
#if GP_ONE_ROW
      __builtin_amdgcn_sched_barrier(0);
#endif
    }
    const size_t tail = (size_t)((wave + 8 * h) * 16 + (GP_EMIT_LANE >> 2)) * GP_SLD + GP_ROWS + (GP_EMIT_LANE & 3) * 4;
    *(bf16x4*)(GP_EMIT_ST + tail) = (bf16x4){0, 0, 0, 0};
    if (GP_EMIT_BOTH) *(bf16x4*)(GP_EMIT_SR + tail) = (bf16x4){0, 0, 0, 0};
  }
}
