// Row statistics of the Gram-pair tile, a fragment of a forward kernel's body (gram_pair.h explains why a fragment).  Lane (g, n) holds rows 4 g + r
// of its wave's strips at columns 16 J + n; a row is 13 accumulators x the 16 lanes of a group.  Leaves at / as scaled into the base-2 domain with
// -inf at columns >= N, and hands every row i, in its lane n == 0, the base-2 log-sum-exps lt / ls of the two Grams' rows and the row's term.
//   reads    : f32x4 at[2][GP_TILES], as[2][GP_TILES]; int N, wave, n, g; bool two
//   GP_STATS_SC2_T, GP_STATS_SC2_S        log2(e) x the teacher's / the student's Gram scale
//   GP_STATS_ADD_TERM(acc, t, s, lt, ls)  statement: acc += the term of one live column (t, s: the scaled Gram elements)
//   GP_STATS_PUT(i, lt, ls, term)         statement, lane n == 0 only: term = the row's sum / log2(e)
//   GP_ONE_ROW                            1: a scheduling barrier behind every row -- interleaved rows cost registers that a kernel at its
//                                         register limit has no room for
#pragma unroll
for (int h = 0; h < 2; ++h) {
  if (h == 0 || two) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = (wave + 8 * h) * 16 + 4 * g + r;
      float mt = -INFINITY, ms = -INFINITY;
#pragma unroll
      for (int J = 0; J < GP_TILES; ++J) {
        const bool valid = J * 16 + n < N;
        at[h][J][r] = valid ? at[h][J][r] * GP_STATS_SC2_T : -INFINITY;
        as[h][J][r] = valid ? as[h][J][r] * GP_STATS_SC2_S : -INFINITY;
        mt = fmaxf(mt, at[h][J][r]);
        ms = fmaxf(ms, as[h][J][r]);
      }
      mt = group16_max(mt);
      ms = group16_max(ms);
      float st = 0.f, ss = 0.f;
#pragma unroll
      for (int J = 0; J < GP_TILES; ++J) {
        st += __builtin_amdgcn_exp2f(at[h][J][r] - mt);
        ss += __builtin_amdgcn_exp2f(as[h][J][r] - ms);
      }
      const float lt = mt + log2f(group16_sum(st)), ls = ms + log2f(group16_sum(ss));
      float term = 0.f;
#pragma unroll
      for (int J = 0; J < GP_TILES; ++J)
        if (J * 16 + n < N) GP_STATS_ADD_TERM(term, at[h][J][r], as[h][J][r], lt, ls)
      term = group16_sum(term) * (1.0f / LOG2E);
      if (n == 0) GP_STATS_PUT(i, lt, ls, term)
#if GP_ONE_ROW
      __builtin_amdgcn_sched_barrier(0);
#endif
    }
  }
}
