"""cal_qkv_loss / cal_qkv_loss2 / soft_cross_entropy (utils/losses.py:37-41, 247-292) on the 16-bit path: a float64 restatement with its analytic
backward, and a per-element first-order error model of the kernel sequence (csrc/qkvce.hip), derived from the inputs alone -- no factor is fitted to
what a GPU gave.

The data model: a PACKED qkv buffer x [B, N, 3 D] (component i in columns [i D, (i + 1) D), head h of it at 64 h) whose values are exactly
representable in the 16-bit storage type, so the inputs carry no error.  X_i, the [B, N, D] rows of component i:
    layout "view"    the reference's q.contiguous().view(B, N, H * 64) of q [B, H, N, 64]: chunk m of row r is head (r H + m) / N, token (r H + m) % N
    layout "tokens"  the head-concatenated token rows
The sequence and where it rounds (u = 2^-8: bf16 unit roundoff, e = 2^-23: one fp32 ulp, charged per MFMA-accumulated product as in _hid_model):
    Z_ij  = X_i X_j^T / 8                 exact products, fp32 accumulation over D; held as z log2(e) / 8
    lse   row and column log-sum-exps     fp32, v_exp_f32 / log2
    term  = sum_j P_t (lse_s - z_s)       fp32; the loss is the fixed-order fp32 sum of the terms / (P L B N)
    S_ij  = bf16(c (e^{zs-lsr} + e^{zs-lsc} - e^{zt-ltr} - e^{zt-ltc}))     four fp32 exponentials that cancel where student and teacher agree (the
                                          E_249 term of _attn_model.relation_bounds, here with row and column parts), ONE bf16 rounding
    d_i   = bf16(up * sum_j S_ij X_j)     fp32 accumulation over up to 3 x 224 keys, the device scalar in fp32, ONE bf16 rounding
Every bound is absolute and per element.

`emulate` is an honest fp32 CPU emulation of that sequence; its `mutate` switches are four wrong kernels that the bounds must NOT hold."""
import math

import torch

from _tail_model import ratio  # noqa: F401  (worst |got - ref| / bound over every element; callers use it as QM.ratio)
from oracle.detgen import det_array

F32, F64, BF16, F16 = torch.float32, torch.float64, torch.bfloat16, torch.float16
E32 = 2.0 ** -23         # one fp32 ulp
U = 2.0 ** -8            # bf16 unit roundoff
TINY = 2.0 ** -126
PAIRS_SELF = [(0, 0), (1, 1), (2, 2)]
PAIRS_CROSS = [(i, j) for i in range(3) for j in range(3)]

# (B, N, Ds, Dt) of the GPU test: rows straddling heads for both models at the smallest size; one head (the layouts coincide); 17; three images of
# 198 rows; 197 (one token), 208 (the most the kernels take); the compacted student
CASES = [(1, 5, 128, 192), (2, 16, 64, 128), (2, 17, 128, 256), (3, 198, 384, 768), (1, 197, 384, 768), (2, 208, 384, 768), (2, 198, 256, 768)]
REGIMES = ("sharp", "flat", "same", "negative", "f16")


def pairs(cross):
    return PAIRS_CROSS if cross else PAIRS_SELF


def quantize(x, dtype=BF16):
    return x.to(dtype).to(F64)


def inputs(B, N, Ds, Dt, regime):
    """(student packed [B, N, 3 Ds], teacher packed [B, N, 3 Dt], upstream) as float64 holding 16-bit values:
    sharp     std 0.5: the self Grams' softmaxes are near one-hot
    flat      std 0.05: near-uniform softmaxes
    same      teacher == student (Dt = Ds): the gradient is 0, the loss the mean entropy
    negative  std 0.5 with upstream -0.75
    f16       the teacher buffer holds IEEE f16"""
    tag = f"qkvce/{regime}/{B}x{N}"
    std = 0.05 if regime == "flat" else 0.5
    s = quantize(torch.from_numpy(det_array(tag + f"/s{Ds}", (B, N, 3 * Ds), std=std)))
    if regime == "same":
        return s, s.clone(), 0.5
    t = torch.from_numpy(det_array(tag + f"/t{Dt}", (B, N, 3 * Dt), std=std))
    t = quantize(t, F16 if regime == "f16" else BF16)
    return s, t, (-0.75 if regime == "negative" else 0.5)


def golden_inputs():
    """the two layer pairs of tests/golden/qkvce.npz as (q, k, v) tuples of fp32 [B, H, N, 64]: B = 2, N = 5, student 2 heads, teacher 3 -- the
    smallest shape where rows straddle heads for both models"""
    def qkv(tag, H):
        return tuple(torch.from_numpy(det_array(f"qkvce/golden/{tag}/{c}", (2, H, 5, 64), std=0.5)) for c in "qkv")
    return [qkv(f"s{i}", 2) for i in range(2)], [qkv(f"t{i}", 3) for i in range(2)]


def golden_ce_inputs():
    return [(torch.from_numpy(det_array(f"qkvce/golden/ce{i}/p", shp, std=2.0)), torch.from_numpy(det_array(f"qkvce/golden/ce{i}/t", shp, std=2.0)))
            for i, shp in enumerate([(3, 7), (2, 5, 5)])]


def pack(qkv):
    """(q, k, v) of [B, H, N, 64] -> packed [B, N, 3 H 64]"""
    B, H, N, C = qkv[0].shape
    return torch.cat([x.permute(0, 2, 1, 3).reshape(B, N, H * C) for x in qkv], dim=-1)


def unpack(x, H):
    B, N, W = x.shape
    D = W // 3
    return tuple(x[:, :, i * D:(i + 1) * D].reshape(B, N, H, D // H).permute(0, 2, 1, 3) for i in range(3))


# ------------------------------------------------------------------------------------------------ the chunk map
def chunk_map(N, H, layout, device=None):
    """(head, token) of chunk m of row r, as two [N, H] integer tensors: the statement of the issue, g = r H + m -> (g // N, g % N)"""
    r, m = torch.meshgrid(torch.arange(N, device=device), torch.arange(H, device=device), indexing="ij")
    if layout == "tokens":
        return m, r
    g = r * H + m
    return g // N, g % N


def rows(x, comp, layout):
    """X_comp [B, N, D] of a packed buffer under the layout, by the chunk map (differentiable gather)"""
    B, N, W = x.shape
    D = W // 3
    H = D // 64
    h, n = chunk_map(N, H, layout, x.device)
    f = x[:, :, comp * D:(comp + 1) * D].reshape(B, N, H, 64)
    return f[:, n, h, :].reshape(B, N, D)


def scatter_rows(dX, layout):
    """the transpose of rows(): d of one component's column block [B, N, D] from dX [B, N, D]"""
    B, N, D = dX.shape
    H = D // 64
    h, n = chunk_map(N, H, layout, dX.device)
    out = torch.zeros(B, N, H, 64, dtype=dX.dtype, device=dX.device)
    out[:, n, h, :] = dX.reshape(B, N, H, 64)
    return out.reshape(B, N, D)


# ------------------------------------------------------------------------------------------------ float64 restatement
def soft_ce(p, t):
    """utils/losses.py:37-41"""
    return (-torch.softmax(t, -1) * torch.log_softmax(p, -1)).sum(-1).mean()


def reference_form(stu, tea, cross):
    """the reference's two functions verbatim in torch ops of any dtype, on lists of (q, k, v) [B, H, N, C] tuples: .contiguous().view()"""
    total = 0.
    for s, t in zip(stu, tea):
        B, Hs, N, Cs = s[0].shape
        _, Ht, _, Ct = t[0].shape
        for i, j in pairs(cross):
            zs = (s[i].contiguous().view(B, N, Hs * Cs) / Cs ** 0.5) @ s[j].contiguous().view(B, N, Hs * Cs).transpose(1, 2)
            zt = (t[i].contiguous().view(B, N, Ht * Ct) / Ct ** 0.5) @ t[j].contiguous().view(B, N, Ht * Ct).transpose(1, 2)
            total = total + soft_ce(zs, zt)
    return total / (len(pairs(cross)) * len(stu))


def definition(xs, xt, cross, layout, layers=1):
    """the loss of one packed pair by the definition (autograd-able)"""
    total = 0.
    for i, j in pairs(cross):
        zs = rows(xs, i, layout) @ rows(xs, j, layout).transpose(1, 2) / 8.0
        zt = rows(xt, i, layout) @ rows(xt, j, layout).transpose(1, 2) / 8.0
        total = total + soft_ce(zs, zt)
    return total / (len(pairs(cross)) * layers)


def restate(xs, xt, cross, layout, layers=1, upstream=1.0):
    """float64 values of what the kernels produce for one packed pair, backward analytic: with c = upstream / (P L B N 8),
    S_ij = c (dP_rows + dP_cols) of Z_ij (i <= j), S_ji = S_ij^T, dX_i = sum_j S_ij X_j, scattered back through the chunk map.
    -> dict(loss, terms[(i, j)] [B, N], S[(i, j)] [B, N, N] for the ordered pairs the mode uses, d [B, N, 3 Ds], Xs, and per-Gram softmax pieces)"""
    xs, xt = xs.to(F64), xt.to(F64)
    B, N, W = xs.shape
    Ds = W // 3
    P = 9 if cross else 3
    c = upstream / (P * layers * B * N * 8.0)
    Xs = [rows(xs, i, layout) for i in range(3)]
    Xt = [rows(xt, i, layout) for i in range(3)]
    terms, S, grams = {}, {}, {}
    for i, j in ([(0, 0), (1, 1), (2, 2)] + ([(0, 1), (0, 2), (1, 2)] if cross else [])):
        zs, zt = Xs[i] @ Xs[j].transpose(1, 2) / 8.0, Xt[i] @ Xt[j].transpose(1, 2) / 8.0
        lsr, ltr = torch.logsumexp(zs, 2, keepdim=True), torch.logsumexp(zt, 2, keepdim=True)
        lsc, ltc = torch.logsumexp(zs, 1, keepdim=True), torch.logsumexp(zt, 1, keepdim=True)
        Psr, Ptr, Psc, Ptc = torch.exp(zs - lsr), torch.exp(zt - ltr), torch.exp(zs - lsc), torch.exp(zt - ltc)
        terms[(i, j)] = (Ptr * (lsr - zs)).sum(2)
        S[(i, j)] = c * ((Psr - Ptr) + (Psc - Ptc))
        if i != j:
            terms[(j, i)] = (Ptc * (lsc - zs)).sum(1)
            S[(j, i)] = S[(i, j)].transpose(1, 2)
        grams[(i, j)] = dict(zs=zs, zt=zt, lsr=lsr, ltr=ltr, lsc=lsc, ltc=ltc, Psr=Psr, Ptr=Ptr, Psc=Psc, Ptc=Ptc)
    loss = sum(t.sum() for t in terms.values()) / (P * layers * B * N)
    d = torch.cat([scatter_rows(sum(S[(i, j)] @ Xs[j] for j in range(3) if (i, j) in S), layout) for i in range(3)], dim=-1)
    return dict(loss=loss, terms=terms, S=S, d=d, Xs=Xs, Xt=Xt, grams=grams, c=c, P=P)


def cal(stu, tea, cross, layout="view"):
    """float64 (loss, [packed student gradients]) of the list form on lists of (q, k, v) tuples"""
    L = len(stu)
    parts = [restate(pack(s), pack(t), cross, layout, L) for s, t in zip(stu, tea)]
    return sum(p["loss"] for p in parts), [p["d"] for p in parts]


# ------------------------------------------------------------------------------------------------ the error model
def _arg_err(Xi, Xj, z, lse, D):
    """bound of the absolute error (in nats) of the fp32 argument z - lse of an exponential, = the relative error of the exponential: the Gram is an
    fp32 sum of D exact products (one ulp per accumulated product, + 2 for the scale and the base change), the log-sum-exp carries at most the
    worst argument error of its row / column (a weighted mean of them) plus the roundings of its own sum and logarithm, the subtraction one ulp
    of each side, v_exp_f32 one: + 8 for those."""
    ez = E32 * ((D + 2) * (Xi.abs() @ Xj.abs().transpose(1, 2) / 8.0 + z.abs()))
    dim = 2 if lse.shape[2] == 1 else 1
    return ez + ez.amax(dim, keepdim=True) + E32 * (2 * z.abs() + 2 * lse.abs() + 8)


def bounds(xs, xt, cross, layout, layers=1, upstream=1.0):
    """(restate(...), dict(loss=bound, terms={pair: bound}, S={pair: bound}, d=bound)) for the 16-bit path"""
    r = restate(xs, xt, cross, layout, layers, upstream)
    B, N, W = xs.shape
    Ds, Dt = W // 3, xt.shape[2] // 3
    c = abs(r["c"])
    eS, eT = {}, {}
    for (i, j), g in r["grams"].items():
        Esr = _arg_err(r["Xs"][i], r["Xs"][j], g["zs"], g["lsr"], Ds)
        Esc = _arg_err(r["Xs"][i], r["Xs"][j], g["zs"], g["lsc"], Ds)
        Etr = _arg_err(r["Xt"][i], r["Xt"][j], g["zt"], g["ltr"], Dt)
        Etc = _arg_err(r["Xt"][i], r["Xt"][j], g["zt"], g["ltc"], Dt)
        # S: four exponentials, three additions and the scale in fp32 (relative to the TERMS: they cancel), then ONE bf16 rounding
        terms4 = g["Psr"] + g["Psc"] + g["Ptr"] + g["Ptc"]
        e32 = c * (g["Psr"] * Esr + g["Psc"] * Esc + g["Ptr"] * Etr + g["Ptc"] * Etc + 4 * E32 * terms4)
        eS[(i, j)] = e32 + U * (r["S"][(i, j)].abs() + e32) + TINY
        # row terms: sum_j P_t (lse_s - z_s): P_t's relative error, the difference's absolute one, an fp32 sum of N products through 4 tree levels
        a = (g["lsr"] - g["zs"]).abs()
        eT[(i, j)] = (g["Ptr"] * (Etr * a + Esr)).sum(2) + E32 * (N / 16 + 8) * (g["Ptr"] * a).sum(2) + TINY
        if i != j:
            eS[(j, i)] = eS[(i, j)].transpose(1, 2)
            a = (g["lsc"] - g["zs"]).abs()
            eT[(j, i)] = (g["Ptc"] * (Etc * a + Esc)).sum(1) + E32 * (N / 16 + 16) * (g["Ptc"] * a).sum(1) + TINY
    # the loss: the fixed-order sum of the P B N terms -- ceil(n / 8192) additions in a lane, 3 + 6 tree levels, 16 at the end -- and the scale
    n = r["P"] * B * N
    k = math.ceil(n / 8192) + 3 + 6 + 16 + 2
    tot = sum(t.abs().sum() for t in r["terms"].values())
    e_loss = (sum(e.sum() for e in eT.values()) + k * E32 * tot) / (r["P"] * layers * B * N)
    # d_i = bf16(up sum_j S_ij X_j): the inputs are exact; fp32 accumulation over 224 keys per product, at most three products, the scalar, ONE rounding
    e_d = []
    for i in range(3):
        js = [j for j in range(3) if (i, j) in r["S"]]
        lin = sum(eS[(i, j)] @ r["Xs"][j].abs() for j in js)
        mag = sum((r["S"][(i, j)].abs() + eS[(i, j)]) @ r["Xs"][j].abs() for j in js)
        exact = sum(r["S"][(i, j)] @ r["Xs"][j] for j in js).abs()
        e32 = lin + E32 * (224 * len(js) + 2) * mag
        e_d.append(scatter_rows(e32 + U * (exact + e32) + TINY, layout))
    return r, dict(loss=e_loss, terms=eT, S=eS, d=torch.cat(e_d, dim=-1))


def soft_ce_bounds(p, t, upstream=1.0):
    """soft_cross_entropy on fp32 rows: float64 (loss, d_predicts) and their bounds.  The inputs are fp32 and exact; the kernels hold x log2(e) in fp32
    (one rounding of the product: relative 2^-24 of |x|), one wave per row with C / 64 additions in a lane and 6 tree levels."""
    p64, t64 = p.to(F64).reshape(-1, p.shape[-1]), t.to(F64).reshape(-1, p.shape[-1])
    R, C = p64.shape
    lp, lt = torch.logsumexp(p64, 1, keepdim=True), torch.logsumexp(t64, 1, keepdim=True)
    Pp, Pt = torch.exp(p64 - lp), torch.exp(t64 - lt)
    a = (lp - p64).abs()
    terms = (Pt * (lp - p64)).sum(1)
    depth = C / 64 + 8

    def arg(x, l):
        e = E32 * (2 * x.abs() + 2)
        return e + e.amax(1, keepdim=True) + E32 * (2 * l.abs() + depth + 8)
    Ep, Et = arg(p64, lp), arg(t64, lt)
    e_terms = (Pt * (Et * a + Ep)).sum(1) + E32 * depth * (Pt * a).sum(1)
    k = math.ceil(R / 8192) + 3 + 6 + 16 + 2
    e_loss = (e_terms.sum() + k * E32 * terms.abs().sum()) / R + TINY
    sc = upstream / R
    dp = (Pp - Pt) * sc
    e_dp = abs(sc) * (Pp * Ep + Pt * Et + 3 * E32 * (Pp + Pt)) + TINY
    return terms.sum() / R, dp.reshape(p.shape), e_loss, e_dp.reshape(p.shape)


# ------------------------------------------------------------------------------------------------ CPU emulation
MUTATIONS = ("half", "identity", "kl", "batchmean")


def emulate(xs, xt, cross, layout, layers=1, upstream=1.0, mutate=None):
    """The kernel sequence in fp32 torch on the CPU: fp32 Grams and log-sum-exps, the four exponentials in fp32, S rounded once to bf16,
    d = bf16(up * fp32 sum).  mutate (each an honest WRONG kernel):
        half       the transposed / column half of S lost: S_ij = c dP_rows
        identity   the identity chunk map where the view map is asked for
        kl         KL instead of CE: the teacher's entropy dropped from the loss
        batchmean  the mean over B instead of B N
    -> dict(loss fp32 scalar, d float64 [B, N, 3 Ds] holding bf16 values)"""
    B, N, W = xs.shape
    P = 9 if cross else 3
    lay = "tokens" if mutate == "identity" else layout
    denom = P * layers * B * (1 if mutate == "batchmean" else N)
    coef = torch.tensor(1.0 / (denom * 8.0), dtype=F32)
    Xs = [rows(xs, i, lay).to(F32) for i in range(3)]
    Xt = [rows(xt, i, lay).to(F32) for i in range(3)]
    S, total = {}, torch.zeros((), dtype=F32)
    eighth = torch.tensor(0.125, dtype=F32)
    for i, j in ([(0, 0), (1, 1), (2, 2)] + ([(0, 1), (0, 2), (1, 2)] if cross else [])):
        zs, zt = (Xs[i] @ Xs[j].transpose(1, 2)) * eighth, (Xt[i] @ Xt[j].transpose(1, 2)) * eighth
        lsr, ltr = torch.logsumexp(zs, 2, keepdim=True), torch.logsumexp(zt, 2, keepdim=True)
        lsc, ltc = torch.logsumexp(zs, 1, keepdim=True), torch.logsumexp(zt, 1, keepdim=True)
        Ptr, Ptc = torch.exp(zt - ltr), torch.exp(zt - ltc)

        def term(Pt, ls, lt, dim):
            if mutate == "kl":
                return (Pt * ((zt - lt) - (zs - ls))).sum(dim).sum()
            return (Pt * (ls - zs)).sum(dim).sum()
        total = total + term(Ptr, lsr, ltr, 2)
        if i != j:
            total = total + term(Ptc, lsc, ltc, 1)
        if mutate == "half":
            s32 = (torch.exp(zs - lsr) - Ptr) * coef
        else:
            s32 = (torch.exp(zs - lsr) + torch.exp(zs - lsc) - Ptr - Ptc) * coef
        S[(i, j)] = s32.to(BF16).to(F32)
        if i != j:
            S[(j, i)] = S[(i, j)].transpose(1, 2)
    loss = total * torch.tensor(1.0 / denom, dtype=F32)
    up = torch.tensor(upstream, dtype=F32)
    d = torch.cat([scatter_rows(((sum(S[(i, j)] @ Xs[j] for j in range(3) if (i, j) in S)) * up).to(BF16).to(F64), lay) for i in range(3)], dim=-1)
    return dict(loss=loss, d=d)
