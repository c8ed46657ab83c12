// The body of cls_loss_kernel (losses.hip), included once per instantiation: CLS_LOSS_KERNEL names it; CLS_LOSS_DET == 0 is the default path's kernel
// (the workgroups' shares meet in the three scalars by fp32 atomics), 1 deterministic mode's: `loss` is then the workspace, [workgroups][3].
__global__ __launch_bounds__(1024) void CLS_LOSS_KERNEL(const ClsArgs a) {
  __shared__ float red[16][2];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int C = a.C;
  float base_acc = 0.f, dist_acc = 0.f;
  for (int b = blockIdx.x * 16 + wv; b < a.B; b += 16 * gridDim.x) {
    float xo[MAXC_PER_LANE], xk[MAXC_PER_LANE], xt[MAXC_PER_LANE], yy[MAXC_PER_LANE];
    int n = 0;
#pragma unroll
    for (int i = 0; i < MAXC_PER_LANE; ++i) {
      const int c = lane + i * 64;
      if (c < C) {
        xo[i] = a.lo[(size_t)b * C + c];
        xk[i] = a.lk[(size_t)b * C + c];
        xt[i] = a.lt ? a.lt[(size_t)b * C + c] : 0.f;
        yy[i] = a.y[(size_t)b * C + c];
        n = i + 1;
      } else {
        xo[i] = xk[i] = xt[i] = -INFINITY;
        yy[i] = 0.f;
      }
    }
    // n differs between lanes only in the last partial group: make the loop bound wave-uniform and
    // rely on the -inf / 0 padding above
    n = (C + 63) / 64;
    float mo, lseo;
    row_lse(xo, n, 1.0f, mo, lseo);
    float ysum = 0.f, bl = 0.f;
#pragma unroll
    for (int i = 0; i < MAXC_PER_LANE; ++i)
      if (i < n && lane + i * 64 < C) {
        ysum += yy[i];
        bl -= yy[i] * (xo[i] - lseo);
      }
    ysum = wave_sum(ysum);
    base_acc += wave_sum(bl);
    const float wbase = (a.kind == 0 ? 1.0f : 1.0f - a.alpha) / (float)a.B;
#pragma unroll
    for (int i = 0; i < MAXC_PER_LANE; ++i) {
      const int c = lane + i * 64;
      if (i < n && c < C) a.dlo[(size_t)b * C + c] = (expf(xo[i] - lseo) * ysum - yy[i]) * wbase;
    }
    if (a.kind == 2) {  // hard: CE(kd, argmax teacher)   utils/losses.py:153
      float best = -INFINITY;
      int bi = 0x7fffffff;
#pragma unroll
      for (int i = 0; i < MAXC_PER_LANE; ++i) {
        const int c = lane + i * 64;
        if (i < n && c < C && xt[i] > best) { best = xt[i]; bi = c; }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {   // max value, ties -> lowest index (torch.argmax on CPU)
        const float ob = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
      }
      float mk, lsek;
      row_lse(xk, n, 1.0f, mk, lsek);
      float xsel = 0.f;
#pragma unroll
      for (int i = 0; i < MAXC_PER_LANE; ++i)
        if (i < n && lane + i * 64 == bi) xsel = xk[i];
      xsel = wave_sum(xsel);
      dist_acc += lsek - xsel;
      const float wd = a.alpha / (float)a.B;
#pragma unroll
      for (int i = 0; i < MAXC_PER_LANE; ++i) {
        const int c = lane + i * 64;
        if (i < n && c < C) a.dlk[(size_t)b * C + c] = (expf(xk[i] - lsek) - (c == bi ? 1.f : 0.f)) * wd;
      }
    } else if (a.kind == 1) {  // soft: KL(log_softmax(kd/T) || log_softmax(tea/T)) T^2 / numel   :140-148
      const float it = 1.0f / a.tau;
      float mk, lsek, mt, lset;
      row_lse(xk, n, it, mk, lsek);
      row_lse(xt, n, it, mt, lset);
      float kl = 0.f;
      const float wd = a.alpha * a.tau / ((float)a.B * (float)C);
#pragma unroll
      for (int i = 0; i < MAXC_PER_LANE; ++i) {
        const int c = lane + i * 64;
        if (i < n && c < C) {
          const float la = xk[i] * it - lsek, lb = xt[i] * it - lset;
          kl += expf(lb) * (lb - la);
          a.dlk[(size_t)b * C + c] = (expf(la) - expf(lb)) * wd;
        }
      }
      dist_acc += wave_sum(kl);
    } else {
#pragma unroll
      for (int i = 0; i < MAXC_PER_LANE; ++i) {
        const int c = lane + i * 64;
        if (i < n && c < C) a.dlk[(size_t)b * C + c] = 0.f;
      }
    }
  }
  if (lane == 0) { red[wv][0] = base_acc; red[wv][1] = dist_acc; }
  __syncthreads();
  if (threadIdx.x == 0) {
    float bs = 0.f, ds = 0.f;
    for (int i = 0; i < 16; ++i) { bs += red[i][0]; ds += red[i][1]; }
    bs /= (float)a.B;
    if (a.kind == 2) ds /= (float)a.B;
    else if (a.kind == 1) ds *= a.tau * a.tau / ((float)a.B * (float)C);
#if CLS_LOSS_DET
    a.loss[3 * blockIdx.x + 1] = bs;
    a.loss[3 * blockIdx.x + 2] = ds;
    a.loss[3 * blockIdx.x + 0] = a.kind == 0 ? bs : bs * (1.0f - a.alpha) + ds * a.alpha;
#else
    unsafeAtomicAdd(a.loss + 1, bs);
    unsafeAtomicAdd(a.loss + 2, ds);
    unsafeAtomicAdd(a.loss + 0, a.kind == 0 ? bs : bs * (1.0f - a.alpha) + ds * a.alpha);
#endif
  }
}
