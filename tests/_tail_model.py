"""Float64 statements, first-order elementwise error bounds, fp32 emulations with planted bugs, case lists and seeded inputs for the kernels
behind the C ABI that are neither GEMM, attention, dropout, HSIC nor the optimizer (tests/_optim_model.py): csrc/layernorm.hip + ln_rows.h, elementwise.hip, losses.hip, the index
copies of shrink.hip and the exact-fp32 companions of sgemm.hip.  Plain torch on the CPU; shared by tests/test_tail_model.py (the model itself
under test, no GPU) and tests/test_gpu_tail.py (the kernels under test), which therefore see the same inputs.

Convention of every bound: u = 2^-24 (fp32 unit roundoff) times the sum of the absolute values of the terms that enter an element, times the
number of roundings on the longest path from an input to that element, COUNTED FROM THE KERNEL SOURCE (each count names its lines).  A correctly
rounded operation costs 1; a device transcendental or a division costs 2 (expf, logf, rsqrtf, sqrtf, erff and `/` are documented at <= 1 ulp =
2 u on this target); __expf costs 4.  No factor is put on top, and nothing is fitted to what the kernels deliver.  A fused multiply-add only removes a rounding, so a bound that
counts the product and the sum separately holds whichever contraction the compiler chose.  Stored 16-bit outputs add the unit roundoff of the
stored type, 2^-8 |ref| (bf16: 8 significand bits) or 2^-11 |ref| (f16: 11), and carry the fp32 error through that rounding (factor 1 + 2^-8).
A correct round-to-nearest store comes arbitrarily close to that term on its own, so 16-bit outputs are held below 1, not 0.5, by the emulation.

ratio(got, ref, bound) is the worst |got - ref| / bound over every element; an error where the bound is exactly 0, or a non-finite output, is
inf.  The emulations (`*_emulate`) redo the operations in fp32 torch in an order of their own: they must stay at ratio <= 0.5 -- except on the
SHORT_PATHS below, outputs that are two to five roundings of values of their own magnitude: there the bound is the worst case of a correct
implementation, which some element of a few thousand comes close to, so the emulation is held below 1 on them, as on the 16-bit stores -- and each planted
bug (`mutate=`) must reach ratio >= 1 (or a torch.equal mismatch in the exact-integer cases) on a named output of a named case."""
import math

import torch

BF16, F16, F32, F64 = torch.bfloat16, torch.float16, torch.float32, torch.float64
U = 2.0 ** -24
H_BF16, H_F16 = 2.0 ** -8, 2.0 ** -11          # unit roundoff of the two 16-bit storage types (half an ulp, relative to the value)


def ratio(got, ref, bound):
    """worst |got - ref| / bound over EVERY element (the semantics of _attn_model.ratio): 0 / 0 -> 0, x / 0 -> inf, non-finite output -> inf"""
    got = torch.as_tensor(got).to(F64).cpu()
    ref = torch.as_tensor(ref, dtype=F64).cpu().expand_as(got)
    bound = torch.as_tensor(bound, dtype=F64).cpu().expand_as(got)
    err = (got - ref).abs()
    rt = torch.where(err == 0, torch.zeros_like(err), err / bound)
    rt = torch.where(torch.isfinite(got), rt, torch.full_like(rt, math.inf))
    return float(rt.max()) if rt.numel() else 0.0


# outputs (the names tests/test_tail_model.py gives them) whose bound is a handful of roundings of the output's own magnitude, with the count
SHORT_PATHS = {"dlo": "cls_distill_loss dlogits: where y dominates, the subtraction, wbase (3) and its product: 5",
               "dlk": "cls_distill_loss dlogits_kd: the subtraction, wd (<= 3) and its product, on p at 2 + its log-probability",
               "da": "token_mse da = 2 d inv: 4", "S_f32": "relation_grad S: three additions of four exponentials of 2 + 1 each, times up"}


def stored16(bound, ref, f16=False):
    """the bound of a value that is stored in a 16-bit type after the fp32 computation `bound` describes; f16 values below 2^-14 are subnormal:
    spacing 2^-24, so half of that in absolute terms"""
    return bound * (1 + 2.0 ** -8) + (H_F16 if f16 else H_BF16) * ref.abs() + (2.0 ** -25 if f16 else 0.0)


def _f(v):
    """a python scalar as the fp32 value a `float` argument of the C ABI carries"""
    return float(torch.tensor(v, dtype=F32))


TINY = 2.0 ** -126          # fp32 results below this are subnormal or flushed to zero: an absolute term wherever an exponential can underflow


def gen(*key):
    s = 0
    for k in key:
        s = (s * 1000003 + (hash(k) if not isinstance(k, str) else sum(ord(c) * (i + 1) for i, c in enumerate(k)))) % (2 ** 31 - 1)
    return torch.Generator(device="cpu").manual_seed(s)


def randn(g, *shape):
    return torch.randn(shape, generator=g, dtype=F32)


def randint(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).to(F32)


def r32(x):
    return x.to(F32).to(F64)


# ============================================================================================ LayerNorm (layernorm.hip, ln_rows.h)
LN_DS = (64, 128, 192, 256, 320, 384, 512, 768, 1024)
LN_BAD_DS = (100, 448, 640, 1152)
LN_ROWS = (1, 7, 8, 9, 250)
LN_FWD_CAP_ROWS, LN_BWD_CAP_ROWS = 16384 + 9, 8192 + 9
LN_EPS = 1e-6
LN_FWD_MUTATIONS = ("one_pass_variance",)
LN_BWD_MUTATIONS = ("xh_term_dropped", "neighbour_rstd")
ROWSCALE_MIX = (0.5, 2.0, 0.0, 1.0)


def ln_cases():
    """(D, rows): every width at 250 rows and at one of the small row counts, every small row count at D = 384, the two grid-capped row counts"""
    out = [(D, 250) for D in LN_DS] + [(D, LN_ROWS[i % 4]) for i, D in enumerate(LN_DS)] + [(384, r) for r in LN_ROWS[:4]]
    return out + [(128, LN_BWD_CAP_ROWS), (128, LN_FWD_CAP_ROWS)]


def ln_inputs(D, rows):
    """fp32 CPU tensors.  Row r is of regime r % 5: N(0.5, 2) / mean 1000 std 0.01 / mean -1e4 std 1 / constant 3 / zeros.  dy holds bf16 values."""
    g = gen("ln", D, rows)
    x = randn(g, rows, D)
    reg = torch.arange(rows) % 5
    x = torch.where((reg == 0)[:, None], x * 2 + 0.5, x)
    x = torch.where((reg == 1)[:, None], x * 0.01 + 1000.0, x)
    x = torch.where((reg == 2)[:, None], x - 1e4, x)
    x = torch.where((reg == 3)[:, None], torch.full_like(x, 3.0), x)
    x = torch.where((reg == 4)[:, None], torch.zeros_like(x), x)
    rps = max(1, (rows + 3) // 4)
    return dict(x=x.contiguous(), regime=reg, gamma=1 + 0.1 * randn(g, D), beta=0.1 * randn(g, D), dy=randn(g, rows, D).to(BF16).to(F32),
                dres=randn(g, rows, D), rowscale=torch.tensor(ROWSCALE_MIX, dtype=F32), rows_per_scale=rps,
                dgamma0=randn(g, D), dbeta0=randn(g, D), colsum0=randn(g, D))


def ln_nv(D):
    return (D + 127) // 128


def ln_fwd_ref(x, gamma, beta, eps=LN_EPS):
    """nn.LayerNorm as include/devit_hip.h words it: y = (x - mean) * rstd * gamma + beta, rstd = (var + eps)^-1/2, biased variance"""
    x, gamma, beta = x.to(F64), gamma.to(F64), beta.to(F64)
    mean = x.mean(1)
    d = x - mean[:, None]
    var = (d * d).mean(1)
    rstd = (var + _f(eps)) ** -0.5                      # eps as the fp32 value the entry point receives
    return dict(y=d * rstd[:, None] * gamma + beta, mean=mean, rstd=rstd, xhat=d * rstd[:, None], absdev=d.abs().mean(1))


def ln_fwd_bounds(x, gamma, beta, eps=LN_EPS):
    """-> (reference dict, bounds for mean, rstd, y).  NV = ceil(D / 128) float4 per lane (ln_fwd_kernel, layernorm.hip).
    mean: lines 57-63: (a + b) + (c + d) is 2 roundings, `s +=` NV - 1 more (the first adds to 0), 5 xor-shuffle adds, invD itself is rounded
          (line 45) and multiplies (line 63): n_mean = NV + 8.           |dmean| <= u n_mean mean|x|
    rstd: lines 64-75: d = x - mu carries dmean and one rounding; q is a chain of 4 NV fused multiply-adds per lane (d * d is not rounded apart:
          counted anyway, 1 each) + 5 shuffle adds, times invD (2: invD and the product), plus eps (1): n_q = 4 NV + 8; the relative error of the
          variance is 2 u (d, squared) + n_q u + 2 dmean mean|d| / (var + eps); rsqrtf halves it and adds 2:
                                                                         |drstd| / rstd <= u (2 NV + 7) + dmean mean|d| rstd^2
    y:    line 83: ((x - mu) * rs) * gamma + beta: d (dmean + u |d|), times rs (drstd, 1), times gamma (1), plus beta (1 on |y|):
                                                                         |dy| <= |gamma| (rstd dmean + |xhat| (drstd / rstd + 3 u)) + u |y|"""
    r = ln_fwd_ref(x, gamma, beta, eps)
    D = x.shape[1]
    nv = ln_nv(D)
    e_mean = U * (nv + 8) * x.to(F64).abs().mean(1)
    rel_rstd = U * (2 * nv + 7) + e_mean * r["absdev"] * r["rstd"] ** 2
    e_y = gamma.to(F64).abs() * ((r["rstd"] * e_mean)[:, None] + r["xhat"].abs() * (rel_rstd + 3 * U)[:, None]) + U * r["y"].abs()
    return r, dict(mean=e_mean, rstd=r["rstd"] * rel_rstd, y=e_y)


def ln_fwd_emulate(x, gamma, beta, eps=LN_EPS, mutate=None):
    """fp32 torch in the kernel's algorithm (two passes); mutate one_pass_variance: var = E[x^2] - E[x]^2"""
    assert mutate is None or mutate in LN_FWD_MUTATIONS
    x, gamma, beta = x.to(F32), gamma.to(F32), beta.to(F32)
    invD = torch.tensor(1.0 / x.shape[1], dtype=F32)
    mu = x.sum(1) * invD
    d = x - mu[:, None]
    var = (x * x).sum(1) * invD - mu * mu if mutate else (d * d).sum(1) * invD
    rs = torch.rsqrt(var + torch.tensor(eps, dtype=F32))
    return dict(y=d * rs[:, None] * gamma + beta, mean=mu, rstd=rs)


def ln_bwd_grid(rows):
    return (rows + 7) // 8 if rows < 8 * 1024 else 1024           # layernorm.hip:206


def ln_col_roundings(rows):
    """roundings on the longest path of a column sum of the LayerNorm backward: a half-wave adds its rows in sequence (ln_rows.h:70-71,151: one per
    trip, layernorm.hip:104), the two half-waves of a wave 1 (ln_rows.h:167-169), the four waves 3 (:180), the partials ceil(parts / 32) per
    group and 32 groups in sequence (layernorm.hip:145,152), the accumulate 1 (:154)"""
    grid = ln_bwd_grid(rows)
    trips = (rows + grid * 8 - 1) // (grid * 8)
    return trips + 1 + 3 + (grid + 31) // 32 + 32 + 1


def ln_bwd_ref(x, mean, rstd, gamma, dy, dres=None):
    """dx = dres + rstd (g - mean(g) - xh mean(g xh)), g = dy gamma, xh = (x - mean) rstd with the SAVED mean / rstd (inputs of the call);
    dgamma = sum_r dy xh, dbeta = sum_r dy"""
    x, mean, rstd, gamma, dy = (t.to(F64) for t in (x, mean, rstd, gamma, dy))
    xh = (x - mean[:, None]) * rstd[:, None]
    g = dy * gamma
    m1, m2 = g.mean(1, keepdim=True), (g * xh).mean(1, keepdim=True)
    dxl = rstd[:, None] * (g - m1 - xh * m2)
    dx = dxl if dres is None else dxl + dres.to(F64)
    return dict(dx=dx, dgamma=(dy * xh).sum(0), dbeta=dy.sum(0), xh=xh, g=g, m1=m1, m2=m2, dxl=dxl)


def ln_bwd_bounds(x, mean, rstd, gamma, dy, dres=None, dgamma0=None, dbeta0=None):
    """-> (reference dict, bounds for dx, dgamma, dbeta; dgamma / dbeta of the reference include the accumulated dgamma0 / dbeta0).
    ln_rows.h, LnBwdMath::sums / dx and ln_bwd_row:
    m1 = mean(g):     g = dy * gamma 1 (:69), `s1 +=` 4 NV in sequence (:74), 5 shuffle adds (:132), invD and the product 2 (:81): 4 NV + 8
    m2 = mean(g xh):  xh = (x - mu) * rs 2 (:68), g 1, the product 1 (:75), 4 NV + 5 adds, invD 2: 4 NV + 11
    dx:               rs * (g - m1 - xh * m2) (:82): g 1, xh 2 and the product xh * m2 1 (on |xh m2|), two subtractions (on the sum of the absolute
                      terms T = |g| + |m1| + |xh m2|), the product with rs 1 (on |dx_ln|), the residual add 1 (on |dx|, :145):
                      |d dx| <= rstd (dm1 + |xh| dm2 + 6 u T) + u (|dx_ln| + |dx|)
    dgamma:           terms dy * xh (:70): 3 roundings each, then ln_col_roundings(rows) adds;  dbeta (:71): the adds alone"""
    r = ln_bwd_ref(x, mean, rstd, gamma, dy, dres)
    rows, D = x.shape
    nv = ln_nv(D)
    rs = rstd.to(F64)[:, None]
    e_m1 = U * (4 * nv + 8) * r["g"].abs().mean(1, keepdim=True)
    e_m2 = U * (4 * nv + 11) * (r["g"] * r["xh"]).abs().mean(1, keepdim=True)
    T = r["g"].abs() + r["m1"].abs() + (r["xh"] * r["m2"]).abs()
    e_dx = rs * (e_m1 + r["xh"].abs() * e_m2 + 6 * U * T) + U * (r["dxl"].abs() + r["dx"].abs())
    nc = ln_col_roundings(rows)
    g0 = torch.zeros(D, dtype=F64) if dgamma0 is None else dgamma0.to(F64)
    b0 = torch.zeros(D, dtype=F64) if dbeta0 is None else dbeta0.to(F64)
    dyd = dy.to(F64)
    e_dg = U * (nc + 3) * ((dyd * r["xh"]).abs().sum(0) + g0.abs())
    e_db = U * nc * (dyd.abs().sum(0) + b0.abs())
    r["dgamma"], r["dbeta"] = r["dgamma"] + g0, r["dbeta"] + b0
    return r, dict(dx=e_dx, dgamma=e_dg, dbeta=e_db)


def ln_colsum_bounds(dx_bf16, colsum0=None):
    """the column sums of the RETURNED dx_bf16 (exact terms) -> (float64 sum (+ colsum0), bound): ln_col_roundings adds"""
    v = dx_bf16.to(F64)
    c0 = torch.zeros(v.shape[1], dtype=F64) if colsum0 is None else colsum0.to(F64)
    return v.sum(0) + c0, U * ln_col_roundings(v.shape[0]) * (v.abs().sum(0) + c0.abs())


def ln_bwd_emulate(x, mean, rstd, gamma, dy, dres=None, dgamma0=None, dbeta0=None, mutate=None):
    assert mutate is None or mutate in LN_BWD_MUTATIONS
    x, mean, rstd, gamma, dy = (t.to(F32) for t in (x, mean, rstd, gamma, dy))
    invD = torch.tensor(1.0 / x.shape[1], dtype=F32)
    xh = (x - mean[:, None]) * rstd[:, None]
    g = dy * gamma
    m1, m2 = g.sum(1, keepdim=True) * invD, (g * xh).sum(1, keepdim=True) * invD
    inner = g - m1 if mutate == "xh_term_dropped" else g - m1 - xh * m2
    rs = rstd.roll(1) if mutate == "neighbour_rstd" else rstd
    dx = rs[:, None] * inner
    if dres is not None:
        dx = dx + dres.to(F32)
    dg, db = (dy * xh).sum(0), dy.sum(0)
    return dict(dx=dx, dgamma=dg if dgamma0 is None else dg + dgamma0.to(F32), dbeta=db if dbeta0 is None else db + dbeta0.to(F32))


# ============================================================================================ small strided fp32 GEMM (elementwise.hip:236-267)
SGEMM_KS = (1, 7, 8, 25, 57, 64, 65, 387)
SGEMM_MNS = ((1, 1), (3, 5), (16, 25))
SGEMM_FORMS = ("token", "b_transposed", "a_kmajor")       # the three stride forms ops.py uses
SGEMM_MUTATIONS = ("tail_k_dropped",)


def sgemm_cases():
    """dicts: K, M, N, form, alpha, accumulate, bias, ints.  Every K with a random and an exact-integer case; the (1000, 384) output with K = 3
    takes the second grid-stride trip (M N > 262144)."""
    out = []
    for i, K in enumerate(SGEMM_KS):
        M, N = SGEMM_MNS[i % 3]
        out.append(dict(K=K, M=M, N=N, form=SGEMM_FORMS[i % 3], alpha=(1.0, 0.5)[i % 2], accumulate=bool((i // 2) % 2), bias=i % 3 != 1, ints=False))
        M, N = SGEMM_MNS[(i + 1) % 3]
        out.append(dict(K=K, M=M, N=N, form=SGEMM_FORMS[(i + 1) % 3], alpha=1.0, accumulate=bool(i % 2), bias=i % 2 == 0, ints=True))
    out.append(dict(K=3, M=1000, N=384, form="token", alpha=0.5, accumulate=True, bias=True, ints=False))
    out.append(dict(K=3, M=1000, N=384, form="b_transposed", alpha=1.0, accumulate=False, bias=False, ints=True))
    return out


def sgemm_inputs(c):
    """logical A [M][K], B [N][K], bias [N] or None, C0 [M][N] (what C holds before the call)"""
    g = gen("sgemm", c["K"], c["M"], c["N"], c["form"], c["ints"])
    mk = (lambda *s: randint(g, -3, 3, *s)) if c["ints"] else (lambda *s: randn(g, *s))
    return dict(A=mk(c["M"], c["K"]), B=mk(c["N"], c["K"]), bias=mk(c["N"]) if c["bias"] else None, C0=mk(c["M"], c["N"]))


def sgemm_bounds(A, B, bias, C0, alpha, accumulate):
    """C (+)= alpha A B^T + bias.  Lane p of eight takes k = p, p + 8, ...: ceil(K / 8) fused multiply-adds (lines 250-257), 3 shuffle adds
    (258-260), the product with alpha and the bias add (262), the accumulate (264): ceil(K / 8) + 6 roundings"""
    A, B = A.to(F64), B.to(F64)
    K = A.shape[1]
    b = torch.zeros(B.shape[0], dtype=F64) if bias is None else bias.to(F64)
    c0 = C0.to(F64) if accumulate else torch.zeros_like(C0, dtype=F64)
    ref = alpha * (A @ B.t()) + b + c0
    return ref, U * ((K + 7) // 8 + 6) * (abs(alpha) * (A.abs() @ B.abs().t()) + b.abs() + c0.abs())


def sgemm_emulate(A, B, bias, C0, alpha, accumulate, mutate=None):
    """eight fp32 partial chains per output as the kernel forms them; mutate tail_k_dropped: the loop of line 257 is missing, so lane p stops at
    the last whole 64-step of line 250 (k + 56 < K)"""
    assert mutate is None or mutate in SGEMM_MUTATIONS
    M, K = A.shape
    N = B.shape[0]
    A64, B64 = A.to(F64), B.to(F64)
    parts = []
    for p in range(8):
        kend = K
        if mutate:
            nb = max(0, -(-(K - 56 - p) // 64))
            kend = min(K, p + 64 * nb)
        s = torch.zeros((M, N), dtype=F64)
        for k in range(p, kend, 8):
            s = r32(s + A64[:, k:k + 1] * B64[None, :, k])          # one rounding per fused multiply-add (the product is exact in float64)
        parts.append(s.to(F32))
    s = ((parts[0] + parts[1]) + (parts[2] + parts[3])) + ((parts[4] + parts[5]) + (parts[6] + parts[7]))
    s = s * torch.tensor(alpha, dtype=F32)
    if bias is not None:
        s = s + bias.to(F32)
    return C0.to(F32) + s if accumulate else s


# ============================================================================================ column sums of a bf16 matrix (elementwise.hip:124-178)
COLSUM_MS = (1, 7, 9, 33, 511, 512, 515, 1000)
COLSUM_NS = (8, 256, 264, 384)
COLSUM_MUTATIONS = ("skip_not_applied",)


def colsum_cases():
    """(M, N, row_group, row_skip, accumulate); ld = N + 8 throughout"""
    out = [(M, COLSUM_NS[i % 4], 0, 0, bool(i % 2)) for i, M in enumerate(COLSUM_MS)]
    out += [(M, COLSUM_NS[(i + 2) % 4], 0, 0, bool((i + 1) % 2)) for i, M in enumerate(COLSUM_MS)]
    return out + [(23, 264, 5, 2, False), (23, 8, 5, 2, True), (588, 384, 196, 2, True), (588, 256, 196, 2, False)]


def colsum_phys_row(r, group, skip):
    return r + skip * (r // group + 1) if group > 0 else r


def colsum_inputs(M, N, group, skip):
    """y [physical rows][N + 8] fp32 holding small integers where the kernel reads and NaN in the skipped rows and the pad columns; out0 [N]"""
    g = gen("colsum", M, N, group, skip)
    mp = colsum_phys_row(M - 1, group, skip) + 1
    y = torch.full((mp, N + 8), math.nan, dtype=F32)
    rows = torch.tensor([colsum_phys_row(r, group, skip) for r in range(M)])
    y[rows, :N] = randint(g, -3, 3, M, N)
    return dict(y=y, out0=randint(g, -5, 5, N))


def colsum_ref(y, M, N, group, skip, out0=None, mutate=None):
    """out[n] (+)= sum_m y[phys(m)][n] in int64 (the inputs are integers); mutate skip_not_applied: rows 0 .. M-1 as they lie"""
    assert mutate is None or mutate in COLSUM_MUTATIONS
    rows = torch.arange(M) if mutate else torch.tensor([colsum_phys_row(r, group, skip) for r in range(M)])
    s = y[rows, :N].to(F64).sum(0)
    return s if out0 is None else s + out0.to(F64)


# ============================================================================================ logit loss (losses.hip:23-147)
CLS_BS = (1, 15, 17, 33)
CLS_CS = (10, 64, 65, 1000, 1024)
CLS_VARIANTS = ("std3", "outliers", "soft07", "tie_two_lanes", "tie_one_lane")
CLS_MUTATIONS = ("tie_highest_index", "ysum_taken_as_one")
KIND_NONE, KIND_SOFT, KIND_HARD = 0, 1, 2


def cls_cases():
    """(B, C, kind, alpha, tau, variant): every (B, C) with the three kinds; tau, alpha and the variants spread over them; every variant once
    more with the hard kind at C = 1000 (16 classes per lane) and C = 65"""
    out, i = [], 0
    for B in CLS_BS:
        for C in CLS_CS:
            for kind in (KIND_NONE, KIND_SOFT, KIND_HARD):
                out.append((B, C, kind, (0.5, 0.0, 1.0, 0.5)[i % 4], (1.0, 3.0)[(i // 3) % 2] if kind != KIND_SOFT else (3.0, 1.0)[(i // 3) % 2],
                            CLS_VARIANTS[i % 5]))
                i += 1
    for v in CLS_VARIANTS:
        out += [(17, 1000, KIND_HARD, 0.5, 1.0, v), (33, 65, KIND_HARD, 0.5, 1.0, v), (17, 1000, KIND_SOFT, 0.5, 3.0, v)]
    return out


def cls_inputs(B, C, variant):
    """logits / logits_kd / teacher at std 3; outliers: +-80 entries; soft07: targets sum to 0.7; tie_*: the teacher's row maximum twice, at
    (c, c + 1) or, where C > 64, at (c, c + 64) -- one lane of the kernel -- with the higher index placed first in memory order nowhere: the lower
    index must win"""
    g = gen("cls", B, C, variant)
    lo, lk, lt = 3 * randn(g, B, C), 3 * randn(g, B, C), 3 * randn(g, B, C)
    y = torch.softmax(2 * randn(g, B, C), -1)
    if variant == "outliers":
        for t in (lo, lk, lt):
            t[:, 0] = 80.0
            t[:, C - 1] = -80.0
            t[B // 2, C // 2] = 79.0
    if variant == "soft07":
        y = y * 0.7
    if variant.startswith("tie"):
        step = 64 if (variant == "tie_one_lane" and C > 64) else 1
        for b in range(B):
            c = (5 * b + 3) % (C - step)
            lt[b, c] = lt[b, c + step] = float(lt[b].max()) + 1.0
    return dict(lo=lo, lk=lk, lt=lt, y=y)


def _lse_err(xs, n_lane, scale_roundings):
    """absolute error bound of row_lse (losses.hip:23-35) per row, and the pieces: xs = the scaled logits [B][C] (float64).
    x * inv_t (`scale_roundings`: 0 when inv_t == 1, else 1 / tau is rounded and multiplies: 2, relative to |xs|); x - mx 1 on |xs - mx|; expf 2;
    the sum: n_lane in sequence + 6 shuffle adds (:32-33); logf 2 on |log s|; the final add 1 on |lse| (:34)"""
    mx = xs.amax(1, keepdim=True)
    lse = torch.logsumexp(xs, 1, keepdim=True)
    arg = scale_roundings * xs.abs() + (xs - mx).abs()
    rel_s = U * (arg.amax(1, keepdim=True) + 2 + n_lane + 6)
    e_lse = rel_s + 2 * U * (lse - mx).abs() + U * lse.abs()
    return lse, e_lse


def cls_ref(lo, lk, lt, y, kind, alpha, tau, mutate=None):
    """float64 statement of DistillLoss (include/devit_hip.h): base = mean_b sum_c -y log_softmax(lo); none: total = base; soft: distill =
    sum p_t (log p_t - log p_k) tau^2 / (B C) at temperature tau; hard: distill = CE(lk, argmax lt) (ties -> lowest index);
    total = (1 - alpha) base + alpha distill.  -> loss3, dlo, dlk (+ the pieces the bounds use)"""
    lo, lk, lt, y = (t.to(F64) for t in (lo, lk, lt, y))
    B, C = lo.shape
    lpo = lo - torch.logsumexp(lo, 1, keepdim=True)
    ysum = y.sum(1, keepdim=True)
    base_rows = -(y * lpo).sum(1)
    base = base_rows.mean()
    wb = (1.0 if kind == KIND_NONE else 1.0 - alpha) / B
    dlo = (lpo.exp() * (torch.ones_like(ysum) if mutate == "ysum_taken_as_one" else ysum) - y) * wb
    r = dict(lpo=lpo, ysum=ysum, base_rows=base_rows, wb=wb)
    if kind == KIND_HARD:
        mx = lt.amax(1, keepdim=True)
        ismax = lt == mx
        idx = torch.arange(C).expand(B, C)
        bi = torch.where(ismax, idx, torch.full_like(idx, -1)).amax(1) if mutate == "tie_highest_index" \
            else torch.where(ismax, idx, torch.full_like(idx, C)).amin(1)
        lpk = lk - torch.logsumexp(lk, 1, keepdim=True)
        onehot = torch.nn.functional.one_hot(bi, C).to(F64)
        dist_rows = -(lpk * onehot).sum(1)
        dist = dist_rows.mean()
        wd = alpha / B
        dlk = (lpk.exp() - onehot) * wd
        r.update(lpk=lpk, onehot=onehot, dist_rows=dist_rows, wd=wd, bi=bi)
    elif kind == KIND_SOFT:
        la = lk / tau - torch.logsumexp(lk / tau, 1, keepdim=True)
        lb = lt / tau - torch.logsumexp(lt / tau, 1, keepdim=True)
        dist_rows = (lb.exp() * (lb - la)).sum(1)
        dist = dist_rows.sum() * tau * tau / (B * C)
        wd = alpha * tau / (B * C)
        dlk = (la.exp() - lb.exp()) * wd
        r.update(la=la, lb=lb, dist_rows=dist_rows, wd=wd)
    else:
        dist = torch.zeros((), dtype=F64)
        dlk = torch.zeros_like(lk)
    total = base if kind == KIND_NONE else (1 - alpha) * base + alpha * dist
    r.update(loss3=torch.stack([total, base, dist]), dlo=dlo, dlk=dlk)
    return r


def cls_bounds(lo, lk, lt, y, kind, alpha, tau):
    """-> (reference dict, bounds loss3 [3], dlo, dlk).  n = ceil(C / 64) classes per lane.  With e_lse from _lse_err:
    log-probability la = x - lse:    e_la = (scale roundings) u |xs| + e_lse + u |la|          (:72, :121)
    probability p = expf(la):        relative e_la + 2 u                                        (:80, :108, :122-123)
    ysum:                            n + 6 adds (:71, :74)
    dlo = (p ysum - y) wbase (:80):  p ysum (rel(p) + (n + 6) u + u) + u (p ysum + y), then wbase = (1 - alpha) / B (:76: 3) and its product (1): 4 u |dlo|
    dlk hard (:108):                 (p - 1hot) wd: wd p rel(p) + u wd (p + 1hot) + 3 u |dlk|;   soft (:123): wd (pa rel(pa) + pt rel(pt)) + u wd (pa + pt)
                                     + 4 u |dlk| (wd = alpha tau / (B C): 3, the product 1)
    row losses:  base (:72) sum_c y (e_la + u |la|) + (n + 6) u sum_c y |la|;  hard (:103) e_lse + u (|lse| + |x_sel|);
                 soft (:122) sum_c pt ((e_lb + 2 u + u) |lb - la| + e_lb + e_la + u |lb - la|) + (n + 6) u sum_c pt |lb - la|
    scalars (:135-145): a wave adds its rows (1 per row here: one trip), thread 0 adds 16 waves, the normalisation (/ B: 2; soft: tau tau / (B C): 5),
                 ceil(B / 16) atomic adds;  total = bs (1 - alpha) + ds alpha: 4 more on the absolute terms"""
    r = cls_ref(lo, lk, lt, y, kind, alpha, tau)
    lo64, lk64, lt64, y64 = (t.to(F64) for t in (lo, lk, lt, y))
    B, C = lo.shape
    n = (C + 63) // 64
    nblk = (B + 15) // 16
    n_scalar = 1 + 16 + 5 + nblk
    _, e_lse_o = _lse_err(lo64, n, 0)
    lpo = r["lpo"]
    e_la = e_lse_o + U * lpo.abs()
    p = lpo.exp()
    pys = p * r["ysum"]
    e_dlo = r["wb"] * (pys * (e_la + 2 * U + (n + 7) * U) + U * (pys + y64) + TINY) + 4 * U * r["dlo"].abs()
    e_base_rows = (y64 * (e_la + U * lpo.abs())).sum(1) + (n + 6) * U * (y64 * lpo.abs()).sum(1)
    e_base = e_base_rows.sum() / B + U * n_scalar * r["base_rows"].abs().sum() / B
    e_dist = torch.zeros((), dtype=F64)
    e_dlk = torch.zeros_like(lk64)
    if kind == KIND_HARD:
        lsek, e_lse_k = _lse_err(lk64, n, 0)
        lpk = r["lpk"]
        e_lak = e_lse_k + U * lpk.abs()
        pk = lpk.exp()
        e_dlk = r["wd"] * (pk * (e_lak + 2 * U) + U * (pk + r["onehot"]) + TINY) + 3 * U * r["dlk"].abs()
        xsel = (lk64 * r["onehot"]).sum(1, keepdim=True)
        e_rows = (e_lse_k + U * (lsek.abs() + xsel.abs()))[:, 0]
        e_dist = e_rows.sum() / B + U * n_scalar * r["dist_rows"].abs().sum() / B
    elif kind == KIND_SOFT:
        sr = 0 if tau == 1.0 else 2
        _, e_lse_k = _lse_err(lk64 / tau, n, sr)
        _, e_lse_t = _lse_err(lt64 / tau, n, sr)
        la, lb = r["la"], r["lb"]
        e_la_k = sr * U * (lk64 / tau).abs() + e_lse_k + U * la.abs()
        e_lb_t = sr * U * (lt64 / tau).abs() + e_lse_t + U * lb.abs()
        pa, pt = la.exp(), lb.exp()
        e_dlk = r["wd"] * (pa * (e_la_k + 2 * U) + pt * (e_lb_t + 2 * U) + U * (pa + pt) + 2 * TINY) + 4 * U * r["dlk"].abs()
        diff = (lb - la).abs()
        e_rows = (pt * ((e_lb_t + 3 * U) * diff + e_lb_t + e_la_k + U * diff)).sum(1) + (n + 6) * U * (pt * diff).sum(1)
        sc = tau * tau / (B * C)
        e_dist = sc * e_rows.sum() + U * n_scalar * sc * (pt * diff).sum()
    base, dist = r["loss3"][1], r["loss3"][2]
    if kind == KIND_NONE:
        e_total = e_base
    else:
        e_total = (1 - alpha) * e_base + alpha * e_dist + 4 * U * (abs(1 - alpha) * base.abs() + abs(alpha) * dist.abs())
    return r, dict(loss3=torch.stack([e_total, e_base, e_dist]), dlo=e_dlo, dlk=e_dlk)


def cls_emulate(lo, lk, lt, y, kind, alpha, tau, mutate=None):
    """the kernel's operations in fp32 torch; mutations: tie_highest_index (the tie goes to the highest index), ysum_taken_as_one"""
    assert mutate is None or mutate in CLS_MUTATIONS
    lo, lk, lt, y = (t.to(F32) for t in (lo, lk, lt, y))
    B, C = lo.shape
    f = lambda v: torch.tensor(v, dtype=F32)

    def lse_of(x, it):
        xs = x * it
        mx = xs.amax(1, keepdim=True)
        return xs, mx + torch.log(torch.exp(xs - mx).sum(1, keepdim=True))

    xo, lseo = lse_of(lo, f(1.0))
    ysum = torch.ones((B, 1), dtype=F32) if mutate == "ysum_taken_as_one" else y.sum(1, keepdim=True)
    base = (-(y * (xo - lseo)).sum(1)).sum() / f(float(B))
    wb = (f(1.0) if kind == KIND_NONE else f(1.0) - f(alpha)) / f(float(B))
    dlo = (torch.exp(xo - lseo) * ysum - y) * wb
    dist = f(0.0)
    dlk = torch.zeros_like(lk)
    if kind == KIND_HARD:
        mx = lt.amax(1, keepdim=True)
        idx = torch.arange(C).expand(B, C)
        bi = torch.where(lt == mx, idx, torch.full_like(idx, -1)).amax(1) if mutate == "tie_highest_index" \
            else torch.where(lt == mx, idx, torch.full_like(idx, C)).amin(1)
        xk, lsek = lse_of(lk, f(1.0))
        onehot = torch.nn.functional.one_hot(bi, C).to(F32)
        dist = (lsek[:, 0] - (xk * onehot).sum(1)).sum() / f(float(B))
        dlk = (torch.exp(xk - lsek) - onehot) * (f(alpha) / f(float(B)))
    elif kind == KIND_SOFT:
        it = f(1.0) / f(tau)
        xk, lsek = lse_of(lk, it)
        xt, lset = lse_of(lt, it)
        la, lb = xk - lsek, xt - lset
        wd = f(alpha) * f(tau) / (f(float(B)) * f(float(C)))
        dlk = (torch.exp(la) - torch.exp(lb)) * wd
        dist = (torch.exp(lb) * (lb - la)).sum() * (f(tau) * f(tau) / (f(float(B)) * f(float(C))))
    total = base if kind == KIND_NONE else base * (f(1.0) - f(alpha)) + dist * f(alpha)
    return dict(loss3=torch.stack([total, base, dist]), dlo=dlo, dlk=dlk)


# ============================================================================================ token MSE (losses.hip:261-279)
MSE_NS = (1, 1023, 1025, 5460)


def mse_inputs(n):
    g = gen("mse", n)
    return dict(a=randn(g, n), b=randn(g, n) * 0.5 + 0.25, loss0=torch.tensor([1.5], dtype=F32))


def mse_bounds(a, b, loss0=None):
    """loss (+)= mean((a - b)^2), da = 2 (a - b) / n.  d 1, d * d 2 more (relative to d^2: 3); ceil(n / 1024) adds per thread (:266-268), 6 shuffle
    adds, 16 waves in sequence (:276), inv = 1 / n and its product 3 (:265, :277), the accumulate 1;  da: d 1, inv 2, the product 1 (2 d is exact)"""
    a, b = a.to(F64), b.to(F64)
    n = a.numel()
    d = a - b
    l0 = 0.0 if loss0 is None else float(loss0)
    ref = (d * d).mean() + l0
    cnt = 3 + (n + 1023) // 1024 + 6 + 16 + 3 + 1
    return dict(loss=ref, da=2 * d / n), dict(loss=U * cnt * ((d * d).mean() + abs(l0)), da=4 * U * (2 * d / n).abs())


def mse_emulate(a, b, loss0=None):
    a, b = a.to(F32), b.to(F32)
    d = a - b
    inv = torch.tensor(1.0, dtype=F32) / torch.tensor(float(a.numel()), dtype=F32)
    loss = (d * d).sum() * inv
    return dict(loss=loss if loss0 is None else loss + loss0.to(F32)[0], da=2.0 * d * inv)


# ============================================================================================ relation loss on given Grams (losses.hip:151-258)
REL_NS = (1, 3, 198, 256)
REL_BS = (1, 3)
REL_HDS = ((64, 64), (64, 32))            # (head_dim_t, head_dim_s)


def rel_cases():
    """(B, N, hd_t, hd_s, scale name): flat = features at std 0.25, unit = std 1 (both softmaxes on the diagonal)"""
    out, i = [], 0
    for N in REL_NS:
        for B in REL_BS:
            for sc in ("flat", "unit"):
                out.append((B, N, *REL_HDS[i % 2], sc))
                i += 1
    return out


def rel_inputs(B, N, hd_t, hd_s, scale):
    """symmetric fp32 Grams [B][N][N] of random bf16 features with 2 heads of hd_t / hd_s (the products the GEMM would deliver, rounded to fp32)"""
    g = gen("rel", B, N, hd_t, hd_s, scale)
    std = 0.25 if scale == "flat" else 1.0
    ft = (randn(g, B, N, 2 * hd_t) * std).to(BF16).to(F64)
    fs = (randn(g, B, N, 2 * hd_s) * std).to(BF16).to(F64)
    gt, gs = (ft @ ft.transpose(1, 2)).to(F32), (fs @ fs.transpose(1, 2)).to(F32)
    gt, gs = torch.maximum(gt, gt.transpose(1, 2)), torch.maximum(gs, gs.transpose(1, 2))        # symmetric to the bit
    return dict(gram_t=gt, gram_s=gs)


def _rel_scaled(gram, hd):
    """(float64 scaled Gram with the fp32 factor the entry point computes, roundings of the scaling relative to |t|): 1 / sqrtf(hd) (losses.hip:313)
    is exact for hd = 64; otherwise sqrtf 2, the division 2; the product 1 (:171)"""
    inv = float(torch.tensor(1.0, dtype=F32) / torch.sqrt(torch.tensor(float(hd), dtype=F32)))
    exact = math.sqrt(hd) == int(math.sqrt(hd))
    return gram.to(F64) * (1.0 / math.sqrt(hd)), (1 if exact else 5), inv


def rel_stats_bounds(gram_t, gram_s, hd_t, hd_s):
    """-> (ref dict lse_t, lse_s, row_kl [B][N], loss, bounds).  One wave per row, 4 columns per lane (rel_stats_kernel):
    lse:     as _lse_err with n_lane = 4 and the scaling roundings above
    a = t - lse (:189): e_a = sr u |t| + e_lse + u |a|
    row_kl = sum_j expf(a_t) (a_t - a_s) (:190): per term pt ((e_at + 2 u + 1 u) |diff| + e_at + e_as + u |diff|), 4 adds per lane + 6 shuffle adds
    loss (fixed_order_reduce_kernel, reduce.h): ceil(n / 8192) adds per slot, 3 tree adds, 6 shuffle adds, 16 waves, 1 / B and the product 3"""
    B, N, _ = gram_t.shape
    t, srt, _ = _rel_scaled(gram_t, hd_t)
    s, srs, _ = _rel_scaled(gram_s, hd_s)
    t2, s2 = t.reshape(B * N, N), s.reshape(B * N, N)
    lt, e_lt = _lse_err(t2, 4, srt)
    ls, e_ls = _lse_err(s2, 4, srs)
    at, as_ = t2 - lt, s2 - ls
    e_at = srt * U * t2.abs() + e_lt + U * at.abs()
    e_as = srs * U * s2.abs() + e_ls + U * as_.abs()
    pt = at.exp()
    diff = (at - as_).abs()
    kl = (pt * (at - as_)).sum(1)
    e_kl = (pt * ((e_at + 3 * U) * diff + e_at + e_as + U * diff)).sum(1) + (4 + 6) * U * (pt * diff).sum(1)
    n = B * N
    cnt = (n + 8191) // 8192 + 3 + 6 + 16 + 3
    ref = dict(lse_t=lt.view(B, N), lse_s=ls.view(B, N), row_kl=kl.view(B, N), loss=kl.sum() / B)
    bnd = dict(lse_t=e_lt.view(B, N), lse_s=e_ls.view(B, N), row_kl=e_kl.view(B, N), loss=e_kl.sum() / B + U * cnt * (pt * diff).sum() / B)
    return ref, bnd


def rel_feature_loss_bounds(fs, ft, hd_t, hd_s):
    """The loss of ops.RelationLossFn from the 16-bit FEATURES fs [B][N][Ds], ft [B][N][Dt] (float64): the statement of rel_stats_bounds on the exact
    Grams, and its bound plus what the Grams' own error can move: a Gram entry is an fp32 sum of D exact products, |dR| <= u (D + 2) |f||f|^T in any
    order (the convention of _attn_model's E_S), and to first order
        d loss / d t_ik = pt_ik ((log pt - log ps)_ik - KL_i) / B,      d loss / d s_ik = (ps_ik - pt_ik) / B       (t, s: the scaled Grams)
    -> (loss, bound)"""
    B = fs.shape[0]
    gt, gs = ft @ ft.transpose(1, 2), fs @ fs.transpose(1, 2)
    ref, bnd = rel_stats_bounds(gt, gs, hd_t, hd_s)
    ct, cs = 1.0 / math.sqrt(hd_t), 1.0 / math.sqrt(hd_s)
    e_t = U * (ft.shape[-1] + 2) * ct * (ft.abs() @ ft.abs().transpose(1, 2))
    e_s = U * (fs.shape[-1] + 2) * cs * (fs.abs() @ fs.abs().transpose(1, 2))
    lpt, lps = torch.log_softmax(gt * ct, -1), torch.log_softmax(gs * cs, -1)
    pt, ps = lpt.exp(), lps.exp()
    d_t = pt * ((lpt - lps) - ref["row_kl"][..., None])
    extra = ((d_t.abs() * e_t).sum() + ((ps - pt).abs() * e_s).sum()) / B
    return ref["loss"], bnd["loss"] + extra


def rel_stats_emulate(gram_t, gram_s, hd_t, hd_s):
    B, N, _ = gram_t.shape
    it = torch.tensor(1.0, dtype=F32) / torch.sqrt(torch.tensor(float(hd_t), dtype=F32))
    is_ = torch.tensor(1.0, dtype=F32) / torch.sqrt(torch.tensor(float(hd_s), dtype=F32))
    t, s = gram_t.to(F32) * it, gram_s.to(F32) * is_

    def lse(x):
        mx = x.amax(-1, keepdim=True)
        return mx + torch.log(torch.exp(x - mx).sum(-1, keepdim=True))

    lt, ls = lse(t), lse(s)
    at, as_ = t - lt, s - ls
    kl = (torch.exp(at) * (at - as_)).sum(-1)
    return dict(lse_t=lt[..., 0], lse_s=ls[..., 0], row_kl=kl, loss=kl.sum() * (torch.tensor(1.0, dtype=F32) / torch.tensor(float(B), dtype=F32)))


def rel_grad_bounds(gram_t, gram_s, lse_t, lse_s, upstream, hd_t, hd_s, bf16_out):
    """S = G + G^T with the GIVEN row log-sum-exps (inputs of devit_relation_grad, exact fp32 values):
    S_ij = (e^{rs - ls_i} + e^{rs - ls_j} - e^{rt - lt_i} - e^{rt - lt_j}) up,  up = upstream / (B sqrt(hd_s))   (rel_grad_kernel :240-249)
    each exponential: the scaling (sr, on |r|), the subtraction 1 on |r - l|, expf 2; three additions on the sum of the four terms;
    up: coef = 1 / (B sqrtf(hd_s)) 5 (:330), times upstream 1 (:240), the product 1: 7 u |S|.  -> (S [B][N][N], bound)"""
    B, N, _ = gram_t.shape
    t, srt, _ = _rel_scaled(gram_t, hd_t)
    s, srs, _ = _rel_scaled(gram_s, hd_s)
    lt, ls = lse_t.to(F64), lse_s.to(F64)
    up = (1.0 if upstream is None else float(upstream)) / (B * math.sqrt(hd_s))
    terms, errs = [], []
    for r, l, sr, sign in ((s, ls[:, :, None], srs, 1), (s, ls[:, None, :], srs, 1), (t, lt[:, :, None], srt, -1), (t, lt[:, None, :], srt, -1)):
        e = torch.exp(r - l)
        terms.append(sign * e)
        errs.append(e * (U * (sr * r.abs() + (r - l).abs()) + 2 * U))
    S = sum(terms) * up
    e_S = abs(up) * (sum(errs) + 3 * U * sum(x.abs() for x in terms) + 4 * TINY) + 7 * U * S.abs()
    e_S = e_S
    return S, (stored16(e_S, S) if bf16_out else e_S)


def rel_grad_emulate(gram_t, gram_s, lse_t, lse_s, upstream, hd_t, hd_s, bf16_out):
    B = gram_t.shape[0]
    f = lambda v: torch.tensor(float(v), dtype=F32)
    rt, rs = gram_t.to(F32) * (f(1) / torch.sqrt(f(hd_t))), gram_s.to(F32) * (f(1) / torch.sqrt(f(hd_s)))
    up = f(1.0 if upstream is None else upstream) * (f(1) / (f(B) * torch.sqrt(f(hd_s))))
    lt, ls = lse_t.to(F32), lse_s.to(F32)
    v = (torch.exp(rs - ls[:, :, None]) + torch.exp(rs - ls[:, None, :]) - torch.exp(rt - lt[:, :, None]) - torch.exp(rt - lt[:, None, :])) * up
    return v.to(BF16) if bf16_out else v


# ============================================================================================ exact-fp32 companions (sgemm.hip)
SOFTMAX_ROWS = (1, 5)
SOFTMAX_COLS = (1, 63, 65, 198)


def softmax_inputs(rows, ncols):
    """S [rows][ncols] at std 4 with +-1e4 entries in the last row (scale 0.125 -> +-1250); dP at std 1"""
    g = gen("softmax", rows, ncols)
    S = randn(g, rows, ncols) * 4
    S[rows - 1, 0] = 1e4
    if ncols > 1:
        S[rows - 1, ncols - 1] = -1e4
        S[rows - 1, ncols // 2] = 1e4 - 3.0
    return dict(S=S, dP=randn(g, rows, ncols), scale=0.125)


def softmax_bounds(S, scale):
    """P = softmax(scale S), lse (softmax_rows_kernel, sgemm.hip:89-101): row * scale 1 on |xs|, - mx 1 on |xs - mx|, expf 2; the sum ceil(ncols / 64)
    in sequence + 6 shuffle adds; the division 2;  lse = mx + logf(sum): rel(sum) + 2 u |log sum| + u |lse|"""
    xs = S.to(F64) * _f(scale)
    n = (S.shape[1] + 63) // 64
    mx = xs.amax(1, keepdim=True)
    arg = U * (xs.abs() + (xs - mx).abs())
    lse = torch.logsumexp(xs, 1, keepdim=True)
    rel_s = arg.amax(1, keepdim=True) + U * (2 + n + 6)
    P = torch.exp(xs - lse)
    return dict(P=P, lse=lse[:, 0]), dict(P=P * (arg + 2 * U + rel_s + 2 * U) + TINY, lse=(rel_s + 2 * U * (lse - mx).abs() + U * lse.abs())[:, 0])


def softmax_bwd_bounds(P, dP, scale):
    """dS = scale P (dP - sum_j P dP) from the GIVEN fp32 P (sgemm.hip:103-112): the dot: products 1, ceil(ncols / 64) + 6 adds; the subtraction 1 on
    |dP| + |dot|; scale * p and the product 2 on |dS|"""
    P, dP = P.to(F64), dP.to(F64)
    n = (P.shape[1] + 63) // 64
    dot = (P * dP).sum(1, keepdim=True)
    e_dot = U * (n + 7) * (P * dP).abs().sum(1, keepdim=True)
    sc = _f(scale)
    dS = sc * P * (dP - dot)
    return dS, abs(sc) * P * (e_dot + U * (dP.abs() + dot.abs())) + 2 * U * dS.abs()


def softmax_emulate(S, scale):
    xs = S.to(F32) * torch.tensor(scale, dtype=F32)
    mx = xs.amax(1, keepdim=True)
    e = torch.exp(xs - mx)
    s = e.sum(1, keepdim=True)
    return dict(P=e / s, lse=(mx + torch.log(s))[:, 0])


def gemm_f32_bound(absprod, alpha_abs, extra_abs, K):
    """sgemm_kernel (sgemm.hip:31-69): K fused multiply-adds in k order (:48), alpha * batch_scale 1 and its product 1, the bias add 1 (:64), the
    accumulate 1 (:69): K + 4 roundings over alpha sum|a b| + |bias| + |C_old|"""
    return U * (K + 4) * (alpha_abs * absprod + extra_abs)


def gelu64(v):
    return 0.5 * v * (1 + torch.erf(v / math.sqrt(2.0)))


def dgelu64(v):
    return 0.5 * (1 + torch.erf(v / math.sqrt(2.0))) + v * torch.exp(-0.5 * v * v) / math.sqrt(2 * math.pi)


def gelu_bound(v, e_v):
    """0.5 x (1 + erff(x c)) (devit_common.h:86): z = x c 2 (c and the product) with erf'(z) |z| <= 0.5: u; erff 2 on |erf| <= 1: 4 u; 1 + erf 1 on <= 2:
    2 u -> 7 u on the bracket, times 0.5 |x|; the two products 2 on |gelu|; the input's error through |gelu'| <= 1.13"""
    return 3.5 * U * v.abs() + 2 * U * gelu64(v).abs() + dgelu64(v).abs() * e_v


def dgelu_bound(x):
    """gelu'(x) = 0.5 (1 + erff) + x pdf, pdf = 0.3989 __expf(-0.5 x x) (devit_common.h:97-98): the bracket 7 u / 2; the argument of __expf 2 roundings
    relative to x^2 / 2 and __expf itself 4: x pdf (x^2 u + 4 u) <= 0.46 * 2 u + 4 u |x pdf|, the products 2 on |x pdf|; the add 1 on <= 1.13"""
    xp = (x * torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi)).abs()
    return 3.5 * U + 0.92 * U + 6 * U * xp + 1.13 * U
