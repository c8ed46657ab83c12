"""Float64 statements, first-order elementwise error bounds, fp32 emulations with planted bugs, case tables and seeded inputs for the ranking kernels
of the shrink stage (csrc/hsic.hip: seven kernels behind devit_hsic_target, devit_hsic_scores and devit_hsic_head_pairs) -- the family
tests/_tail_model.py leaves out.  Plain torch, device-agnostic (the statements and bounds run on whatever device their arguments live on); shared by
tests/test_hsic_model.py (the model itself under test, no GPU) and tests/test_gpu_hsic.py (the kernels under test), which therefore see the same
inputs.  U, TINY, ratio and gen are _tail_model's, and so is the convention of every bound: u = 2^-24 times the sum of the absolute values of the
terms that enter an element times the number of roundings on the longest path to it, COUNTED FROM THE KERNEL SOURCE (each count names its lines of
hsic.hip); a correctly rounded operation costs 1, `/` and a libm transcendental 2, the hardware exponential (v_exp_f32) 4; a fused multiply-add is
counted as its product and its sum.  No factor on top, nothing fitted to what the kernels deliver.

Every stage is held on its own, against the float64 statement applied to the fp32 values the stage in front of it produced (the workspace as read
back, the kmix1 as read back, the W that was handed in): a defect of one stage cannot hide in, or be blamed on, another.
    pack        ws[u][n][a] = features(X): exact for group == 1 (torch.equal), bounded for group > 1; samples B .. Bp are zero
    pair        kmix1 from ws, per element; rel = sum kmix1 o W and act = sum |ws| from the device's own kmix1 / ws (double reductions: the
                bound is the final fp32 rounding, the fp32 pair additions inside act and a counted 2^-53 term on sum |terms|)
    target      W from the logits / probabilities, per element
    head_pairs  red from the device's own kmix1 (double throughout)
Units are laid out [units][N][B] everywhere here (the workspace's layout), kernels [units][B][B].

The emulations (`*_emulate`) redo a stage in fp32 torch in an order of their own and must stay at ratio <= 0.5 -- below 1 on SHORT_PATHS -- and each
planted bug (`mutate=`) must reach ratio >= 1, an inf ratio (an error over a zero bound, a non-finite output) or a torch.equal mismatch on the
named output of the named case in MUTATIONS.  (_tail_model.stored16 has no use here: every output of these kernels is fp32.  sigma16_off drops decimal
places of the literal, 1.3e-5 relatively: a constant off in its last BINARY place or two moves an element by at most 4 u c d2 e^(-c d2) / 5, which lies
inside the (N + 3) u of the d2 chain in front of it at any N -- no bound counted from the source can see it, and none is bent to.)"""
import math

import torch

from _tail_model import BF16, F16, F32, F64, TINY, U, gen, randn, ratio  # noqa: F401  (ratio is re-exported to the two test files)

D53 = 2.0 ** -53                                 # unit roundoff of the double accumulators
TILE, NC, MAX_B, MAX_HEADS = 64, 33, 256, 16     # hsic.hip:28
COEF = (0.5, 0.125, 0.03125, 0.0078125, 0.001953125)          # 1 / (2 s^2), s = 1, 2, 4, 8, 16 (hsic.hip:143-144): powers of two
DTYPES = {"bf16": BF16, "f16": F16, "f32": F32}

# outputs whose bound is a handful of roundings of the output's own magnitude, with the count: the emulation is held below 1 on them
SHORT_PATHS = {"rel": "one fp32 rounding of a double sum: 1 (+ the 2^-53 term)", "red": "one fp32 rounding of a double sum: 1 (+ the 2^-53 term)",
               "act": "the fp32 pair additions and the final rounding: 2", "ws": "group additions and the division, group + 1 in all; 3 at group == 2"}

PAIR_MUTATIONS = ("gram_form_d2", "plain_exp_minus_one", "offdiag_tiles_once", "chunk_tail_token_dropped", "sigma16_off")
PACK_MUTATIONS = ("pad_not_zeroed", "group_mean_by_wrong_count")
TARGET_MUTATIONS = ("no_max_subtraction", "gram_tail_column_dropped", "mean_over_classes")
HEAD_MUTATIONS = ("total_term_dropped", "self_pair_included", "divide_by_H")
# planted bug -> (the case it must be caught on, the output it must be caught on)
MUTATIONS = {"gram_form_d2": ("B64_N3_u6_g1_f32_contig", "kmix1"), "plain_exp_minus_one": ("B64_N3_u6_g1_f32_contig", "kmix1"),
             "offdiag_tiles_once": ("B65_N3_u6_g1_bf16_token_pad", "rel"), "chunk_tail_token_dropped": ("B5_N34_u6_g1_f32_contig", "kmix1"),
             "sigma16_off": ("B64_N3_u6_g1_f32_contig", "kmix1"), "pad_not_zeroed": ("B65_N3_u6_g1_bf16_token_pad", "act"),
             "group_mean_by_wrong_count": ("B129_N34_u6_g8_f32_batch_pad", "ws"), "no_max_subtraction": ("B65_C257_softmax", "W"),
             "gram_tail_column_dropped": ("B65_C257_softmax", "W"), "mean_over_classes": ("B65_C257_softmax", "W"),
             "total_term_dropped": ("B65_N6_u3_g3_f16_token_pad", "red"), "self_pair_included": ("B65_N6_u3_g3_f16_token_pad", "red"),
             "divide_by_H": ("B65_N6_u3_g3_f16_token_pad", "red")}


def padded(B):
    return (B + TILE - 1) // TILE * TILE


def workspace_bytes(B, N, units):
    """devit_hsic_scores_workspace (hsic.hip:277-280)"""
    return units * N * padded(B) * 4


# ============================================================================================ float64 statements (include/devit_hip.h)
def center(K):
    return K - K.mean(-2, keepdim=True) - K.mean(-1, keepdim=True) + K.mean((-2, -1), keepdim=True)


def target(y, softmax):
    """W = center(z z^T), z = p - mean_a p, p = softmax of the rows of y [B][C] (softmax != 0) or the rows themselves"""
    y = y.to(F64)
    p = torch.softmax(y, -1) if softmax else y
    z = p - p.mean(0, keepdim=True)
    return center(z @ z.t())


def features(X, group):
    """X [B][N][units * group] -> [units][N][B]: the mean of `group` consecutive channels"""
    B, N, ch = X.shape
    return X.to(F64).reshape(B, N, ch // group, group).mean(-1).permute(2, 1, 0)


def d2(x):
    """x [units][N][B] -> [units][B][B]: a sum of squared DIFFERENCES, token by token (no [units][N][B][B] tensor)"""
    x = x.to(F64)
    out = torch.zeros((x.shape[0], x.shape[2], x.shape[2]), dtype=F64, device=x.device)
    for n in range(x.shape[1]):
        t = x[:, n, :, None] - x[:, n, None, :]
        out += t * t
    return out


def kmix1(x):
    """Kmix - 1 = 1/5 sum_s expm1(-d2 / (2 s^2))"""
    dd = d2(x)
    return sum(torch.expm1(-c * dd) for c in COEF) / 5.0


def rel(k, W):
    return (k.to(F64) * W.to(F64)[None]).sum((1, 2))


def act(x):
    """sum |x| over tokens and samples; x [units][N][B] (group == 1: the values of X themselves)"""
    return x.to(F64).abs().sum((1, 2))


def red(k):
    """red[h] = 1/(H - 1) sum_{g != h} sum_ab Kmix_h o center(Kmix_g); Kmix or Kmix - 1 on both sides (a constant does not survive the centring,
    and the centred side sums to zero)"""
    k = k.to(F64)
    c = center(k)
    H = k.shape[0]
    return torch.stack([sum((k[h] * c[g]).sum() for g in range(H) if g != h) / (H - 1) for h in range(H)])


# ============================================================================================ bounds
def pack_bounds(X, group):
    """-> (features(X) [units][N][B], bound).  hsic_pack_kernel (hsic.hip:98-113, group == 1) converts and copies: bound 0.  hsic_pack_group_kernel
    (:123-128): `s +=` over the group in sequence (:126: group - 1 roundings, the first adds to 0; the conversions are exact), `/ (float)group` 2
    (:127): group + 1 roundings over mean |x|"""
    ref = features(X, group)
    if group == 1:
        return ref, torch.zeros_like(ref)
    B, N, ch = X.shape
    return ref, U * (group + 1) * X.to(F64).abs().reshape(B, N, ch // group, group).mean(-1).permute(2, 1, 0)


def kmix1_bounds(x):
    """x [units][N][B]: the fp32 features as the pack stage left them -> (kmix1(x), bound), [units][B][B].
    d2 (:185-186): t = a - b 1, squared 2, the product 1 and N additions of non-negative terms in sequence (one chain through all token chunks,
          :160-189): |dd2| <= (N + 3) u d2 (+ N 2^-126 where a square underflows; nothing where d2 == 0: the diagonal and coinciding samples are
          exactly 0)
    through the mix: |d/dd2 expm1(-c d2)| = c exp(-c d2), taken at d2 - dd2 (the mean value lies above it)
    argument t = d2 * -c (:143-144): c is a power of two: exact
    expm1_neg (:134-138), whichever branch t > -0.25 selects -- within c dd2 of -0.25 the computed t may take either, the larger bound holds:
      Taylor (:135): q = 1 + t (1/2 + t (1/6 + ... t / 5040)): the constants 1 / k! are rounded (1), six fused multiply-adds (counted 6 on the
          longest path) over sum |t|^k / (k + 1)! = (e^|t| - 1) / |t|; p = t q 1 on |p|; the series is cut after t^7 / 7!, alternating, so the
          remainder is below |t|^8 / 8! (3.8e-10 at 1/4):          |t| 7 u (e^|t| - 1) / |t| + u |expm1 t| + |t|^8 / 40320
      exp2 (:136): t * LOG2E: LOG2E rounded and the product, 2 relative to |t|; v_exp_f32 4 (+ 2^-126 where it underflows); - 1 1 on |expm1 t|:
                                                               e^t (2 |t| + 4) u + 2^-126 + u |expm1 t|
    the sum (:143-144): 4 additions of terms of one sign, 0.2f rounded and its product (:145): 6 u |kmix1|"""
    x = x.to(F64)
    N = x.shape[1]
    dd = d2(x)
    e_d2 = U * (N + 3) * dd + N * TINY * (dd > 0)
    lo = (dd - e_d2).clamp_min(0)
    ref, bnd = torch.zeros_like(dd), torch.zeros_like(dd)
    for c in COEF:
        t = -c * dd
        a = t.abs()
        em = torch.expm1(t)
        ref += em
        # the Taylor bound is only ever selected at |t| <= 1/4 (+ the band): |t| is cut at 1 so that the unselected values stay finite
        series = torch.where(a > 0, torch.expm1(a.clamp_max(1.0)) / a.clamp(1e-300, 1.0), torch.ones_like(a))
        e_poly = a * 7 * U * series + U * em.abs() + a.clamp_max(1.0) ** 8 / 40320.0
        e_exp = torch.exp(t) * (2 * a + 4) * U + TINY + U * em.abs()
        m = c * e_d2
        branch = torch.where(t > -0.25 + m, e_poly, torch.where(t < -0.25 - m, e_exp, torch.maximum(e_poly, e_exp)))
        bnd += c * torch.exp(-c * lo) * e_d2 + branch
    ref = ref / 5.0
    return ref, bnd / 5.0 + 6 * U * ref.abs()


def rel_bounds(k, W):
    """k [units][B][B], W [B][B]: the fp32 values on the device -> (rel(k, W), bound).  weight * (double)k * (double)W is exact in double (:199:
    24 + 24 bits, the weight a power of two); a thread adds 16 terms per tile over nt (nt + 1) / 2 tiles (:158-207), block_sum_double 6 shuffle
    adds and 3 (:37-41), all in double; one fp32 rounding at the store (:210)"""
    terms = k.to(F64) * W.to(F64)[None]
    ref = terms.sum((1, 2))
    nt = padded(k.shape[1]) // TILE
    n = 16 * nt * (nt + 1) // 2 + 9
    return ref, U * ref.abs() + n * D53 * terms.abs().sum((1, 2))


def act_bounds(ws):
    """ws [units][N][Bp] as read back (all Bp columns are summed: :175 runs on whole diagonal tiles) -> (sum |ws|, bound).  :175: two fp32 pair
    additions per float4, each 1 on its own pair: u sum |x| in all; per chunk of tokens at most ceil(33 * 16 / 256) = 3 trips (:168), two double
    additions each, over ceil(N / 33) chunks and Bp / 64 diagonal tiles, then 9 (:212); one fp32 rounding at the store (:213)"""
    s = ws.to(F64).abs().sum((1, 2))
    n = 6 * ((ws.shape[1] + NC - 1) // NC) * (ws.shape[2] // TILE) + 9
    return s, U * s + U * s + n * D53 * s


def red_bounds(k):
    """k [H][B][B]: the fp32 kmix1 on the device -> (red(k), bound).  hsic_head_pairs_kernel (:218-245) in double throughout: a row sum B
    additions and `/ B` (:227-228), the total 9 and a division (:230-231), per g three additions into c (:240: 3 (H - 1)), the product and
    ceil(B^2 / 256) additions into acc (:236-241), 9 (:243), `/ (H - 1)` (:244); one fp32 rounding at the store"""
    k = k.to(F64)
    H, B = k.shape[0], k.shape[1]
    ref = red(k)
    rm, tot = k.abs().mean(2), k.abs().mean((1, 2))
    absc = k.abs() + rm[:, :, None] + rm[:, None, :] + tot[:, None, None]
    allc = absc.sum(0)
    terms = torch.stack([(k[h].abs() * (allc - absc[h])).sum() for h in range(H)]) / (H - 1)
    n = (B + 1) + 10 + 3 * (H - 1) + 1 + (B * B + 255) // 256 + 9 + 1
    return ref, U * ref.abs() + n * D53 * terms


def target_bounds(y, softmax):
    """y [B][C] fp32 -> (target(y, softmax) [B][B], bound).
    p (hsic_softmax_kernel :45-65): softmax == 0 copies: exact.  Else row[c] - m 1 on |y - m| (an absolute error of the argument, so relative to
        the exponential), expf 2; s is a double sum of those (each term off by u (|y - m| + 2) relatively, so s by their p-weighted mean; the
        double additions, C 2^-53, are left to the Gram's term); inv = (float)(1 / s) 1 (:63), the product 1 (:64):
                                        |dp| <= p u (|y - m| + 4 + sum_c p_c (|y_c - m| + 2)) + 2^-126
    z (hsic_center_columns_kernel :67-76): per pass mean = (float)(double sum / B) 1 on |mean|, z -= mean 1 on |z|.  The first pass carries
        dp and its column mean; the second subtracts the (rounded) mean of what the first left, which is the mean of its ERROR since the true z
        has none: it adds at most that mean again and 1 on |z|:
                                        e1 = dp + mean_a dp + u |mean p| + u |z|,    |dz| <= e1 + mean_a e1 + u |z|
    W (hsic_gram_kernel :78-93): exact products added in double in c order, rounded once (:92):
                                        |dW_ab| <= sum_c (|z_a| dz_b + dz_a |z_b|) + u |W| + C 2^-53 sum_c |z_a z_b|"""
    y = y.to(F64)
    C = y.shape[1]
    if softmax:
        a = (y - y.amax(1, keepdim=True)).abs()
        p = torch.softmax(y, -1)
        e_p = p * U * (a + 4 + (p * (a + 2)).sum(1, keepdim=True)) + TINY
    else:
        p, e_p = y, torch.zeros_like(y)
    mean = p.mean(0, keepdim=True)
    z = p - mean
    e1 = e_p + e_p.mean(0, keepdim=True) + U * mean.abs() + U * z.abs()
    e_z = e1 + e1.mean(0, keepdim=True) + U * z.abs()
    W = center(z @ z.t())
    za = z.abs()
    return W, za @ e_z.t() + e_z @ za.t() + U * W.abs() + C * D53 * (za @ za.t())


# ============================================================================================ fp32 emulations with planted bugs
def pack_emulate(X, group, mutate=None):
    """-> ws [units][N][Bp] fp32.  The group sum in torch's own (pairwise) order.  pad_not_zeroed: samples B .. Bp keep what the workspace held --
    NaN in these tests; group_mean_by_wrong_count: the sum is divided by the number of units"""
    assert mutate is None or mutate in PACK_MUTATIONS
    B, N, ch = X.shape
    units = ch // group
    x = X.to(F32).reshape(B, N, units, group)
    f = x[..., 0] if group == 1 else x.sum(-1) / torch.tensor(float(units if mutate == "group_mean_by_wrong_count" else group), dtype=F32)
    ws = torch.full((units, N, padded(B)), math.nan if mutate == "pad_not_zeroed" else 0.0, dtype=F32)
    ws[:, :, :B] = f.permute(2, 1, 0)
    return ws


def kmix1_emulate(ws, B, mutate=None):
    """ws [units][N][>= B] fp32 -> kmix1 [units][B][B] fp32: all squared differences of a unit at once and torch's sum over the tokens, torch's
    expm1, the five terms added from the widest Gaussian down.  gram_form_d2: d2 = |a|^2 + |b|^2 - 2 <a, b>; plain_exp_minus_one: exp(t) - 1;
    chunk_tail_token_dropped: the last token of a partial chunk behind a full one is not walked (token 33 of N = 34); sigma16_off: the last
    constant loses its last two decimal places (0.0019531 for 0.001953125)"""
    assert mutate is None or mutate in ("gram_form_d2", "plain_exp_minus_one", "chunk_tail_token_dropped", "sigma16_off")
    x = ws[:, :, :B].to(F32)
    units, N, _ = x.shape
    if mutate == "chunk_tail_token_dropped" and N > NC and N % NC:
        x = x[:, :N - 1]
    coef = list(COEF)
    if mutate == "sigma16_off":
        coef[4] = 0.0019531
    out = torch.empty((units, B, B), dtype=F32)
    step = max(1, int(2e7) // (N * B * B))
    for u0 in range(0, units, step):
        xs = x[u0:u0 + step]
        if mutate == "gram_form_d2":
            inner = xs.transpose(1, 2) @ xs
            nrm = torch.diagonal(inner, dim1=1, dim2=2)
            dd = nrm[:, :, None] + nrm[:, None, :] - 2 * inner
        else:
            t = xs[:, :, :, None] - xs[:, :, None, :]
            dd = (t * t).sum(1)
        acc = torch.zeros_like(dd)
        for c in reversed(coef):
            tt = dd * torch.tensor(-c, dtype=F32)
            acc = acc + (torch.exp(tt) - 1 if mutate == "plain_exp_minus_one" else torch.expm1(tt))
        out[u0:u0 + step] = acc * torch.tensor(0.2, dtype=F32)
    return out


def rel_emulate(k, W, mutate=None):
    """sum k o W in float64 in torch's order, rounded once.  offdiag_tiles_once: the 64 x 64 tiles above the diagonal enter with weight 1 for 2
    (the tiles below are never walked)"""
    assert mutate is None or mutate == "offdiag_tiles_once"
    terms = k.to(F64) * W.to(F64)[None]
    if mutate:
        t = torch.arange(k.shape[1]) // TILE
        terms = terms * (t[:, None] <= t[None, :]).to(F64)
    return terms.sum((1, 2)).to(F32)


def act_emulate(ws):
    """|x| added in fp32 pairs along the samples, the pairs in float64"""
    a = ws.to(F32).abs()
    return a.reshape(a.shape[0], a.shape[1], -1, 2).sum(-1).to(F64).sum((1, 2)).to(F32)


def red_emulate(k, mutate=None):
    """pair by pair in float64 with the centring written out on the g side.  total_term_dropped: center() without its + mean of all;
    self_pair_included: g == h enters the sum; divide_by_H"""
    assert mutate is None or mutate in HEAD_MUTATIONS
    k = k.to(F64)
    H = k.shape[0]
    c = k - k.mean(-2, keepdim=True) - k.mean(-1, keepdim=True)
    if mutate != "total_term_dropped":
        c = c + k.mean((-2, -1), keepdim=True)
    out = []
    for h in range(H):
        s = sum((k[h] * c[g]).sum() for g in range(H) if g != h or mutate == "self_pair_included")
        out.append(s / (H if mutate == "divide_by_H" else H - 1))
    return torch.stack(out).to(F32)


def target_emulate(y, softmax, mutate=None):
    """fp32 softmax in torch's order, means through float64 as the kernel takes them, two centring passes, the Gram in float64 rounded once.
    no_max_subtraction: exp(y) / sum exp(y); gram_tail_column_dropped: the classes behind the last whole 256 do not enter the Gram (class 256 of
    C = 257); mean_over_classes: p is centred over its classes instead of over the batch"""
    assert mutate is None or mutate in TARGET_MUTATIONS
    y = y.to(F32)
    C = y.shape[1]
    if softmax:
        e = torch.exp(y if mutate == "no_max_subtraction" else y - y.amax(1, keepdim=True))
        p = e * (1.0 / e.to(F64).sum(1, keepdim=True)).to(F32)
    else:
        p = y
    z = p
    for _ in range(2):
        z = z - z.to(F64).mean(1 if mutate == "mean_over_classes" else 0, keepdim=True).to(F32)
    if mutate == "gram_tail_column_dropped" and C > 256 and C % 256:
        z = z[:, :C - C % 256]
    return (z.to(F64) @ z.to(F64).t()).to(F32)


# ============================================================================================ case tables and seeded inputs
LAYOUTS = ("contig", "token_pad", "batch_pad", "offset", "all")


def _case(B, N, units, group, dt, layout, seam):
    return dict(name=f"B{B}_N{N}_u{units}_g{group}_{dt}_{layout}", B=B, N=N, units=units, group=group, dtype=DTYPES[dt], layout=layout, seam=seam)


def neuron_cases():
    """group == 1: each row crosses one seam with the others at their smallest non-trivial value (6 units: one per feature regime), and one real row"""
    return [_case(2, 3, 6, 1, "bf16", "contig", "smallest batch; 16-bit samples that collide"),
            _case(63, 3, 6, 1, "f16", "contig", "one short of the 64-sample tile"),
            _case(64, 3, 6, 1, "f32", "contig", "exactly one tile: no pad column"),
            _case(65, 3, 6, 1, "bf16", "token_pad", "one sample in the second tile: off-diagonal tiles, 63 pad columns"),
            _case(128, 3, 6, 1, "f16", "contig", "two whole tiles"),
            _case(129, 3, 6, 1, "f32", "batch_pad", "three tiles, the last with one sample"),
            _case(193, 3, 6, 1, "bf16", "contig", "four tiles, the last with one sample"),
            _case(256, 3, 6, 1, "f32", "contig", "HSIC_MAX_B"),
            _case(5, 1, 6, 1, "f32", "contig", "one token"),
            _case(5, 32, 6, 1, "bf16", "contig", "one short of the 33-token chunk"),
            _case(5, 33, 6, 1, "f16", "offset", "exactly one chunk"),
            _case(5, 34, 6, 1, "f32", "contig", "one token in the second chunk"),
            _case(5, 66, 6, 1, "bf16", "contig", "two whole chunks"),
            _case(5, 67, 6, 1, "f32", "offset", "three chunks, the last with one token"),
            _case(65, 34, 6, 1, "f32", "contig", "the tile seam and the chunk seam together"),
            _case(5, 3, 1, 1, "f32", "contig", "one unit"),
            _case(5, 3, 63, 1, "bf16", "token_pad", "one short of the pack kernel's 64 channels: c < units guards"),
            _case(5, 3, 64, 1, "f16", "contig", "exactly 64 channels"),
            _case(5, 3, 65, 1, "f32", "token_pad", "one channel in the second block of channels"),
            _case(5, 3, 130, 1, "bf16", "batch_pad", "three blocks of channels, the last with two"),
            _case(37, 198, 128, 1, "bf16", "all", "a real shape: 198 tokens are six chunks")]


def head_cases():
    """group > 1 (H = units): also what devit_hsic_head_pairs is fed from"""
    return [_case(2, 6, 2, 2, "bf16", "contig", "two heads, two samples, the smallest group"),
            _case(65, 6, 3, 3, "f16", "token_pad", "an odd group; the second tile"),
            _case(129, 34, 6, 8, "f32", "batch_pad", "three tiles, two token chunks"),
            _case(2, 34, 16, 64, "bf16", "offset", "HSIC_MAX_HEADS at the real head width"),
            _case(256, 6, 16, 8, "bf16", "contig", "HSIC_MAX_HEADS at HSIC_MAX_B: the head-pair kernel's whole LDS table")]


def score_cases():
    return neuron_cases() + head_cases()


def case_by_name(name):
    return next(c for c in score_cases() + target_cases() if c["name"] == name)


def separate_constant_columns(x, keep):
    """16-bit rounding makes the samples of a column collide now and then (at B = 2 a whole column): sample 0 of a column that is constant and
    non-zero over the batch moves to a neighbouring representable value -- except where `keep` [N][ch] says the column is constant on purpose"""
    for _ in range(4):
        same = (x == x[:1]).all(0) & (x[0] != 0) & ~keep
        if not bool(same.any()):
            break
        x[0] = torch.where(same, x[0] * 1.0078125, x[0])
    return x


def score_inputs(c):
    """-> dict X [B][N][units * group] (contiguous, the case's element type), W [B][B] fp32, logits [B][25].  The regime of a channel is that of
    its unit, unit % 6:
      0  1.5 randn
      1  30 + 0.3 randn kept as fp32 (the Gram form of d2 cancels); in a 16-bit type 3 + 0.3 randn, where the spread survives the rounding
      2  1e-3 randn: |Kmix - 1| ~ 1e-5 (exp(t) - 1 loses it)
      3  8 randn: the narrow Gaussians underflow, Kmix - 1 -> -0.8 .. -1
      4  all zero: a masked unit -- rel, act and every kmix1 entry exactly 0
      5  1.5 randn with token 0 constant (2.5) over the batch: only differences enter"""
    B, N, units, group = c["B"], c["N"], c["units"], c["group"]
    ch = units * group
    g = gen("hsic", c["name"])
    z = randn(g, B, N, ch)
    r = ((torch.arange(ch) // group) % 6).expand(B, N, ch)
    x = 1.5 * z
    x = torch.where(r == 1, (30.0 if c["dtype"] == F32 else 3.0) + 0.3 * z, x)
    x = torch.where(r == 2, 1e-3 * z, x)
    x = torch.where(r == 3, 8.0 * z, x)
    x = torch.where(r == 4, torch.zeros_like(x), x)
    keep = (r[0] == 5) & (torch.arange(N) == 0)[:, None]
    x = torch.where(keep.expand(B, N, ch), torch.full_like(x, 2.5), x)
    x = separate_constant_columns(x.to(c["dtype"]), keep).contiguous()
    logits = 2 * randn(g, B, 25)
    return dict(X=x, logits=logits, W=target(logits, True).to(F32))


def strides_of(c):
    """(element offset of the base, batch stride, token stride, elements of the whole buffer) of the case's layout"""
    B, N, ch = c["B"], c["N"], c["units"] * c["group"]
    lay = c["layout"]
    sn = ch + (5 if lay in ("token_pad", "all") else 0)
    sb = N * sn + (7 if lay in ("batch_pad", "all") else 0)
    off = 3 if lay in ("offset", "all") else 0
    return off, sb, sn, off + (B - 1) * sb + (N - 1) * sn + ch + 37


def target_cases():
    out = []
    for B, C in ((2, 1), (2, 25), (65, 255), (65, 256), (65, 257), (256, 1000), (256, 25), (65, 1)):
        for sm in (1, 0):
            out.append(dict(name=f"B{B}_C{C}_{'softmax' if sm else 'rows'}", B=B, C=C, softmax=sm))
    return out


def target_inputs(c):
    """y [B][C] fp32: logits at std 2; row 0 holds +80 and -80, row 1 is constant, the last row sits at an offset of +100 (exp overflows without
    the maximum's subtraction).  softmax == 0: the fp32 softmax of those logits, the probabilities the public entry hands over."""
    B, C = c["B"], c["C"]
    y = 2 * randn(gen("hsic_target", B, C), B, C)
    y[0, 0] = 80.0
    y[0, C - 1] = -80.0 if C > 1 else 80.0
    y[1] = 0.75
    y[B - 1] += 100.0
    return y if c["softmax"] else torch.softmax(y.to(F64), -1).to(F32)


def synthetic_kmix1(H=3, B=65):
    """a symmetric zero-diagonal kmix1 [H][B][B] fp32 with entries spread log-uniformly over [-1, -1e-7]"""
    g = gen("hsic_synth", H, B)
    k = -torch.exp(torch.rand((H, B, B), generator=g, dtype=F64) * math.log(1e-7)).to(F32)
    k = torch.triu(k, 1)
    return k + k.transpose(1, 2)
