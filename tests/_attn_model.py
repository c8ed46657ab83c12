"""Reference, first-order error model and rounding-by-rounding emulation of csrc/attention.hip (plain torch, float64; runs on the CPU or on
the GPU, wherever its inputs live).  Shared by tests/test_attention_model.py (the model itself under test, no GPU) and the GPU tests.

Everything is stated per (image, head) on "heads form" tensors [B][H][n][64] float64 that hold the 16-bit inputs exactly:
    q [B][H][NQ][64], k / v [B][H][N][64], dout [B][H][NQ][64], gate [H] or None (all ones), add = (aq, ak, av) or None.
The packed kernels are the case NQ == N; the rows form reads the first NQ <= N query rows, which is the packed computation with dO zero
on the other rows and dQ / O / lse sliced to the first NQ.

reference():  S = c Q K^T, P = softmax(S), O = g P V, lse = logsumexp(S); dV = g P^T dO, dP = dO V^T, delta = rowsum(dO * O),
              dS = P * (g dP - delta), dQ = c dS K, dK = c dS^T Q (+ add).

bounds():     elementwise, first order, no free factor.  u = 2^-8 for bf16 storage (2^-10 for f16), e32 = fp32 eps, chain = N + 64:
    E_S     = e32 * 66 * (c |Q||K|^T + |S|)      relative error of P: scores are fp32 MFMA sums of 64 exact products, p = exp2 of them
    W       = u + E_S                             takes u's place wherever u multiplies a P-weighted sum
    E_O     = |g| (P * W)|V| + u |O|              P rounded before P V; one rounding of the stored output
              (+ |g| N 2^-25 max|V| for f16: P below 2^-14 is subnormal there, absolute error up to 2^-25 each, denominator >= 1)
    E_delta = rowsum(|dO| E_O)                    delta is read from the stored `out`
    E_dS    = W |dS| + P E_delta                  dS rounded before its two products
    E_dV    = |g| (P * W)^T |dO| + u |dV + add| + e32 chain |g| P^T |dO|
    E_dQ    = c E_dS |K| + u |dQ + add| + e32 chain c |dS||K|         (the kernel adds `add` in fp32 and rounds once)
    E_dK    = c E_dS^T |Q| + u |dK + add| + e32 chain c |dS|^T |Q|
    E_lse   = 1e-5 max(1, |lse|)                  the project's existing bar, per element
Where a bound is exactly 0 (a head gated off) the output must be exactly 0: ratio() returns inf for any error there.

emulate():    the same operations with the roundings the kernels document (attention.hip): fp32 scores, c2 = scale * log2(e) in fp32,
              p = exp2(fma(s, c2, -max * c2)), fp32 row sum of the unrounded p, P rounded to the 16-bit type before P V, one rounding
              of o * (gate / sum); backward: p = exp2(fma(s, c2, -lse * log2(e))), delta = fp32 rowsum(dO * stored out) * scale,
              dS = p * fma(dP, gate * scale, -delta) rounded to bf16 before dQ / dK, P rounded to bf16 before dV, dV * gate in fp32,
              `add` added in fp32, one rounding of every stored gradient.  `mutate` plants one of the bugs of MUTATIONS.

Dropout on the softmax (the *_drop kernels): all three take keep (bool or 0/1, [B][H][NQ][N]) and s (the fp32 value of 1 / (1 - p)); with
keep=None they are what they were.  Statement: Pd = P * keep s, O = g Pd V, dV = g Pd^T dO, dP = dO V^T, delta = rowsum(dO * O),
dS = P * (g keep s dP - delta); dQ, dK as above, lse of the UNDROPPED row.  Bounds: _bounds_dropped(); emulation: _emulate_dropped()."""
import math

import torch

BF16, F16, F32, F64 = torch.bfloat16, torch.float16, torch.float32, torch.float64
HD = 64
U_BF16, U_F16 = 2.0 ** -8, 2.0 ** -10
E32 = 2.0 ** -23
LSE_BAR = 1e-5
SLOPE_BAR = 2.0 ** -9
LOG2E_F32 = 1.4426950408889634          # the literals of attention.hip; rounded to fp32 where the kernel does
LN2_F32 = 0.6931471805599453
MUTATIONS = ("dq_drops_last_key", "dk_drops_ds_tile", "dv_drops_p_tile", "delta_from_pregate_out",
             # the *_drop kernels (keep / s given)
             "drop_bwd_mask_other_block", "drop_bwd_mask_pitch_n", "drop_lse_of_dropped_row", "drop_delta_from_undropped_out",
             "drop_dv_scaled_twice", "drop_quad_trade_transposed")


# ------------------------------------------------------------------------------------------ layout
def heads(buf, B, n, H, col0=0):
    """rows [0, B n) of a 2-D buffer, columns col0 + h 64 + e  ->  [B][H][n][64] float64"""
    return buf[: B * n, col0:col0 + H * HD].to(F64).view(B, n, H, HD).permute(0, 2, 1, 3).contiguous()


def rows(x):
    """[B][H][n][64] -> [B n][H 64]"""
    B, H, n, _ = x.shape
    return x.permute(0, 2, 1, 3).reshape(B * n, H * HD)


def split_packed(qkv, B, N, H, dout=None, add=None):
    """packed [B N][3 D] buffers -> the heads-form arguments of reference() / bounds() / emulate()"""
    D = H * HD
    q, k, v = (heads(qkv, B, N, H, j * D) for j in range(3))
    do = None if dout is None else heads(dout, B, N, H)
    ad = None if add is None else tuple(heads(add, B, N, H, j * D) for j in range(3))
    return q, k, v, do, ad


def _gate(gate, H, like):
    g = torch.ones(H, dtype=F64, device=like.device) if gate is None else gate.to(F64).to(like.device)
    return g.view(1, H, 1, 1)


# ------------------------------------------------------------------------------------------ reference
def _keep_scale(keep, s, like):
    """m = keep * s as float64 [B][H][NQ][N]; s is the fp32 value of 1 / (1 - p)"""
    assert s is not None and float(torch.tensor(s, dtype=F32)) == float(s), "s: the fp32 value of 1 / (1 - p)"
    assert keep.shape == like.shape, (keep.shape, like.shape)
    return keep.to(like.device).to(F64) * float(s)


def reference(q, k, v, gate, scale, dout=None, add=None, keep=None, s=None):
    H = q.shape[1]
    g = _gate(gate, H, q)
    S = scale * (q @ k.transpose(-1, -2))
    lse = torch.logsumexp(S, -1)
    P = torch.exp(S - lse[..., None])
    m = None if keep is None else _keep_scale(keep, s, P)
    Pd = P if m is None else P * m
    O = g * (Pd @ v)
    r = dict(S=S, P=P, O=O, lse=lse, g=g)
    if m is not None:
        r.update(Pd=Pd, m=m)
    if dout is not None:
        dV0 = g * (Pd.transpose(-1, -2) @ dout)
        dP = dout @ v.transpose(-1, -2)
        delta = (dout * O).sum(-1, keepdim=True)
        dS = P * (g * dP - delta) if m is None else P * (g * m * dP - delta)
        if m is not None:
            r.update(gmdP=g * m * dP, delta=delta)
        dQ0 = scale * (dS @ k)
        dK0 = scale * (dS.transpose(-1, -2) @ q)
        aq, ak, av = add if add is not None else (0.0, 0.0, 0.0)
        r.update(dS=dS, dQ=dQ0 + aq, dK=dK0 + ak, dV=dV0 + av)
    return r


def bounds(q, k, v, gate, scale, dout=None, add=None, u=U_BF16, f16=False, keep=None, s=None):
    """-> (reference dict, dict of elementwise bounds for O, lse and, with dout, dQ / dK / dV)"""
    r = reference(q, k, v, gate, scale, dout, add, keep, s)
    N = k.shape[2]
    g, P, S = r["g"].abs(), r["P"], r["S"]
    chain = N + 64
    E_S = E32 * 66 * (scale * (q.abs() @ k.abs().transpose(-1, -2)) + S.abs())
    if keep is not None:
        return r, _bounds_dropped(r, q, k, v, scale, dout, u, E_S, chain)
    PW = P * (u + E_S)
    E_O = g * (PW @ v.abs()) + u * r["O"].abs()
    if f16:
        E_O = E_O + g * N * 2.0 ** -25 * v.abs().amax(dim=(-1, -2), keepdim=True)
    b = dict(O=E_O, lse=LSE_BAR * r["lse"].abs().clamp_min(1.0))
    if dout is not None:
        ado = dout.abs()
        E_delta = (ado * E_O).sum(-1, keepdim=True)
        adS = r["dS"].abs()
        E_dS = (u + E_S) * adS + P * E_delta
        b["dV"] = g * (PW.transpose(-1, -2) @ ado) + u * r["dV"].abs() + E32 * chain * g * (P.transpose(-1, -2) @ ado)
        b["dQ"] = scale * (E_dS @ k.abs()) + u * r["dQ"].abs() + E32 * chain * scale * (adS @ k.abs())
        b["dK"] = scale * (E_dS.transpose(-1, -2) @ q.abs()) + u * r["dK"].abs() + E32 * chain * scale * (adS.transpose(-1, -2) @ q.abs())
    return r, b


def _bounds_dropped(r, q, k, v, scale, dout, u, E_S, chain):
    """bounds() for the *_drop kernels (bf16 only): the plain bounds with Pd = P keep s in P's place in every P-weighted sum, and the
    fp32 products dropout adds, each with an e32 of the quantity it scales:
        forward (attention_fwd.inc)   sc = (gate * dk.s) / sum: the product gate * dk.s and the product o * sc that applies it
        dV      (attention_bwd.inc)   pp = p * s in ATTN_DROPPED, and dv * gate at the store
        dS                            dp * s in ATTN_DROPPED and gs = gate * scale, both on the g keep s dP term; delta * scale and
                                      the fma's own rounding on the delta side
    so W = u + E_S + 2 e32 and E_dS gains 2 e32 P (|g keep s dP| + |delta|).  delta is read from the stored (dropped) `out`."""
    g, P, Pd = r["g"].abs(), r["P"], r["Pd"]
    W = u + E_S + 2 * E32
    PW = Pd * W
    E_O = g * (PW @ v.abs()) + u * r["O"].abs()
    b = dict(O=E_O, lse=LSE_BAR * r["lse"].abs().clamp_min(1.0))
    if dout is not None:
        ado = dout.abs()
        E_delta = (ado * E_O).sum(-1, keepdim=True)
        adS = r["dS"].abs()
        E_dS = W * adS + P * E_delta + 2 * E32 * P * (r["gmdP"].abs() + r["delta"].abs())
        b["dV"] = g * (PW.transpose(-1, -2) @ ado) + u * r["dV"].abs() + E32 * chain * g * (Pd.transpose(-1, -2) @ ado)
        b["dQ"] = scale * (E_dS @ k.abs()) + u * r["dQ"].abs() + E32 * chain * scale * (adS @ k.abs())
        b["dK"] = scale * (E_dS.transpose(-1, -2) @ q.abs()) + u * r["dK"].abs() + E32 * chain * scale * (adS.transpose(-1, -2) @ q.abs())
    return b


def ratio(got, ref, bound):
    """worst |got - ref| / bound over EVERY element; an error where the bound is exactly 0 counts as inf, a non-finite output as inf"""
    err = (got.to(F64) - ref).abs()
    rt = torch.where(err == 0, torch.zeros_like(err), err / bound)          # 0 / 0 -> 0, x / 0 -> inf
    rt = torch.where(torch.isfinite(got.to(F64)), rt, torch.full_like(rt, math.inf))
    return float(rt.max())


def slope(got, ref):
    """least-squares gain of got against ref, per head over all images: sum(got ref) / sum(ref ref) -> [H]"""
    got = got.to(F64)
    return (got * ref).sum(dim=(0, 2, 3)) / (ref * ref).sum(dim=(0, 2, 3))


# ------------------------------------------------------------------------------------------ emulation
def _r32(x):
    return x.to(F32).to(F64)


def _r16(x, f16=False):
    return x.to(F32).to(F16 if f16 else BF16).to(F64)       # the kernels round fp32 values


def quad_transposed(keep):
    """the keep bit of (query 4a + r, key 4b + p) taken for (query 4a + p, key 4b + r): what a transposed word trade would give.  Rows past
    NQ repeat the last row (the kernel's clamp), key columns past N are kept (they are masked as padded keys anyway)."""
    B, H, NQ, N = keep.shape
    nq4, n4 = (NQ + 3) & ~3, (N + 3) & ~3
    kp = torch.ones((B, H, nq4, n4), dtype=torch.bool, device=keep.device)
    kp[:, :, :NQ, :N] = keep.bool()
    kp[:, :, NQ:, :N] = keep.bool()[:, :, NQ - 1:NQ, :]
    kp = kp.view(B, H, nq4 // 4, 4, n4 // 4, 4).transpose(3, 5).reshape(B, H, nq4, n4)
    return kp[:, :, :NQ, :N].contiguous()


def emulate(q, k, v, gate, scale, dout=None, add=None, f16=False, mutate=None, keep=None, s=None, keep_bwd=None):
    """-> dict O, lse and, with dout, dQ / dK / dV: float64 tensors holding what the kernels would store (see the module docstring)"""
    assert mutate is None or mutate in MUTATIONS
    if keep is not None:
        assert not f16, "the *_drop kernels are bf16 only"
        return _emulate_dropped(q, k, v, gate, scale, dout, add, mutate, keep, s, keep_bwd)
    assert mutate is None or not mutate.startswith("drop_")
    H, N = q.shape[1], k.shape[2]
    g = _r32(_gate(gate, H, q))
    sc32 = float(torch.tensor(scale, dtype=F32))
    c2 = float(torch.tensor(sc32, dtype=F32) * torch.tensor(LOG2E_F32, dtype=F32))
    s = _r32(q @ k.transpose(-1, -2))                                         # raw scores, fp32 accumulators
    mxs = _r32(s.amax(-1, keepdim=True) * c2)
    p = _r32(torch.exp2(_r32(s * c2 - mxs)))
    psum = _r32(p.sum(-1, keepdim=True))
    lse = _r32(_r32(mxs + _r32(torch.log2(psum))) * float(torch.tensor(LN2_F32, dtype=F32)))
    o32 = _r32(_r16(p, f16) @ v)
    O = _r16(o32 * _r32(g / psum), f16)
    r = dict(O=O, lse=lse[..., 0])
    if dout is None:
        return r
    assert not f16, "the backward is bf16 only"
    lse2 = _r32(lse * float(torch.tensor(LOG2E_F32, dtype=F32)))
    out_for_delta = O
    if mutate == "delta_from_pregate_out":
        out_for_delta = _r16(o32 * _r32(1.0 / psum))
    delta = _r32(_r32((dout * out_for_delta).sum(-1, keepdim=True)) * sc32)
    pb = _r32(torch.exp2(_r32(s * c2 - lse2)))
    dp = _r32(dout @ v.transpose(-1, -2))
    gs = _r32(g * sc32)
    ds = _r32(pb * _r32(dp * gs - delta))
    p16, ds16 = _r16(pb), _r16(ds)
    ds_q, ds_k, p_v = ds16, ds16, p16
    if mutate == "dq_drops_last_key":
        ds_q = ds16.clone()
        ds_q[..., N - 1] = 0
    if mutate == "dk_drops_ds_tile":
        ds_k = ds16.clone()
        ds_k[..., 16:32, 32:48] = 0
    if mutate == "dv_drops_p_tile":
        p_v = p16.clone()
        p_v[..., 16:32, 32:48] = 0
    dq = _r32(ds_q @ k)
    dk = _r32(ds_k.transpose(-1, -2) @ q)
    dv = _r32(_r32(p_v.transpose(-1, -2) @ dout) * g)
    aq, ak, av = add if add is not None else (0.0, 0.0, 0.0)
    r.update(dQ=_r16(dq + aq), dK=_r16(dk + ak), dV=_r16(dv + av))
    return r


def _emulate_dropped(q, k, v, gate, scale, dout, add, mutate, keep, s, keep_bwd):
    """the *_drop kernels (bf16): the fp32 row sum and lse are of the UNDROPPED p, dropped p is zeroed before the bf16 rounding, the
    output is scaled by fp32(fp32(g s) / sum); backward: pp = fp32(p s) or 0 rounded to bf16 for dV, dS = p * fma(fp32(dp s) or 0, gate
    scale, -delta).  keep_bwd: the mask the backward regenerates (the two wrong-mask mutations; default: the forward's)."""
    assert mutate is None or mutate.startswith("drop_"), mutate
    H, N = q.shape[1], k.shape[2]
    g = _r32(_gate(gate, H, q))
    s32 = float(torch.tensor(s, dtype=F32))
    assert s32 == float(s)
    kf = keep.to(q.device).bool()
    sc32 = float(torch.tensor(scale, dtype=F32))
    c2 = float(torch.tensor(sc32, dtype=F32) * torch.tensor(LOG2E_F32, dtype=F32))
    sr = _r32(q @ k.transpose(-1, -2))
    mxs = _r32(sr.amax(-1, keepdim=True) * c2)
    p = _r32(torch.exp2(_r32(sr * c2 - mxs)))
    pd = torch.where(kf, p, torch.zeros_like(p))
    psum = _r32((pd if mutate == "drop_lse_of_dropped_row" else p).sum(-1, keepdim=True))
    lse = _r32(_r32(mxs + _r32(torch.log2(psum))) * float(torch.tensor(LN2_F32, dtype=F32)))
    O = _r16(_r32(_r16(pd) @ v) * _r32(_r32(g * s32) / psum))
    r = dict(O=O, lse=lse[..., 0])
    if dout is None:
        return r
    kb = kf
    if mutate in ("drop_bwd_mask_other_block", "drop_bwd_mask_pitch_n"):
        assert keep_bwd is not None, "these two need the mask the wrong backward would regenerate"
        kb = keep_bwd.to(q.device).bool()
    if mutate == "drop_quad_trade_transposed":
        kb = quad_transposed(kf)
    mb = torch.where(kb, torch.full_like(p, s32), torch.zeros_like(p))
    lse2 = _r32(lse * float(torch.tensor(LOG2E_F32, dtype=F32)))
    out_for_delta = O
    if mutate == "drop_delta_from_undropped_out":
        out_for_delta = _r16(_r32(_r16(p) @ v) * _r32(g / psum))
    delta = _r32(_r32((dout * out_for_delta).sum(-1, keepdim=True)) * sc32)
    pb = _r32(torch.exp2(_r32(sr * c2 - lse2)))
    dp = _r32(dout @ v.transpose(-1, -2))
    gs = _r32(g * sc32)
    pp = _r32(pb * mb)
    ds = _r32(pb * _r32(_r32(dp * mb) * gs - delta))
    p16, ds16 = _r16(pp), _r16(ds)
    dq = _r32(ds16 @ k)
    dk = _r32(ds16.transpose(-1, -2) @ q)
    dv = _r32(_r32(p16.transpose(-1, -2) @ dout) * g)
    if mutate == "drop_dv_scaled_twice":
        dv = _r32(dv * s32)
    aq, ak, av = add if add is not None else (0.0, 0.0, 0.0)
    r.update(dQ=_r16(dq + aq), dK=_r16(dk + ak), dV=_r16(dv + av))
    return r


def attn_keep(seed, block, thr, B, H, N, NQ=None, pitch=None):
    """the keep mask of the *_drop kernels from the numpy mirror: site 1, logical tensor [B H NQ][N] at pitch ceil4(N) -> bool [B][H][NQ][N]"""
    import numpy as np

    import _philox as PH
    NQ = N if NQ is None else NQ
    pitch = (N + 3) & ~3 if pitch is None else pitch
    if pitch % 4 == 0:
        return torch.from_numpy(PH.keep_mask(seed, 1, block, thr, B * H * NQ, N, pitch)).view(B, H, NQ, N)
    # a pitch the header forbids (what a kernel that forgot ceil4 would index): the same counter layout on e = row * pitch + col
    e = np.arange(B * H * NQ, dtype=np.uint64)[:, None] * np.uint64(pitch) + np.arange(N, dtype=np.uint64)[None, :]
    gq = e >> np.uint64(2)
    w = PH.philox4x32_10((gq & PH.MASK, gq >> np.uint64(32), np.uint64(1), np.uint64(block)), (seed & 0xFFFFFFFF, seed >> 32))
    return torch.from_numpy(np.choose((e & np.uint64(3)).astype(np.int64), w) >= np.uint32(thr)).view(B, H, NQ, N)


# ------------------------------------------------------------------------------------------ fixed inputs (CPU generator: the same on every machine)
REGIMES = {"flat": (0.25, 1.0), "unit": (1.0, 1.0), "peaked": (1.0, 4.0)}        # std of qkv, factor on Q
SHAPES = [(2, 198, 6), (3, 197, 2), (2, 208, 3), (2, 192, 6), (2, 193, 12), (4, 17, 2), (4, 16, 1), (5, 1, 2), (2, 64, 16), (2, 33, 3),
          (2, 207, 6)]
GATE_MIX = (0.5, 2.0, 0.0, 1.0)


def packed_cases():
    """every shape with every regime once; gates (None / the 0, 0.5, 1, 2 mix) and dqkv_add spread over them"""
    out = []
    for i, (B, N, H) in enumerate(SHAPES):
        for j, regime in enumerate(REGIMES):
            out.append((B, N, H, regime, (i + j) % 2 == 0, (i + 2 * j) % 3 == 0))
    return out


# the *_drop kernels: (B, N, H, regime, gated (the 0.5, 2, 0, 1 mix: a zero head from H = 3), dqkv_add, p, block)
DROP_SEED = 20240807
DROP_CASES = [(2, 198, 6, "unit", True, True, 0.1, 4), (2, 198, 6, "peaked", True, False, 0.5, 1), (1, 208, 1, "flat", False, True, 0.5, 4),
              (1, 208, 1, "unit", True, False, 0.1, 1), (2, 193, 3, "peaked", True, False, 0.1, 1), (2, 193, 3, "unit", True, True, 0.5, 4),
              (1, 65, 4, "flat", True, True, 0.5, 1), (2, 17, 2, "unit", False, False, 0.1, 4), (1, 5, 2, "peaked", True, True, 0.5, 4),
              (1, 1, 2, "flat", True, False, 0.1, 1), (2, 5, 3, "flat", True, False, 0.1, 1)]


def drop_params(p):
    """(thr, the fp32 value of 1 / (1 - p)) as the header states them"""
    import _philox as PH
    return PH.threshold(p), float(torch.tensor(1.0 / (1.0 - p), dtype=F32))


def gate_mix(H, nonzero=False):
    vals = (1.0, 0.5, 2.0) if nonzero else GATE_MIX
    return torch.tensor([vals[h % len(vals)] for h in range(H)], dtype=F32)


def make_inputs(B, N, H, regime, dtype=BF16, NQ=None):
    """-> dict of CPU tensors in `dtype`: qkv [B N][3 D], dout [B NQ][D], add [B N][3 D] (seeded by the case)"""
    std, qmul = REGIMES[regime]
    D, NQ = H * HD, N if NQ is None else NQ
    gen = torch.Generator(device="cpu").manual_seed(100000 * list(REGIMES).index(regime) + 100 * N + H + 7 * NQ)
    qkv = torch.randn((B * N, 3 * D), generator=gen) * std
    qkv[:, :D] *= qmul
    dout = torch.randn((B * NQ, D), generator=gen)
    add = torch.randn((B * N, 3 * D), generator=gen) * 0.5
    return dict(qkv=qkv.to(dtype), dout=dout.to(dtype), add=add.to(dtype))


def routing_inputs(B, N, H, seed=0):
    """Sign codes +-4 in 64 dims: Q_i = s_i, K_pi(i) = s_i for a seeded permutation pi per (image, head): with scale 1/8 the matching
    score is 128, the others 2 <sigma_i, sigma_j>.  -> dict: qkv [B N][3 D] bf16, dout, perm [B][H][N] (pi), max_other (largest
    non-matching score)."""
    D = H * HD
    gen = torch.Generator(device="cpu").manual_seed(seed + N)
    code = (torch.randint(0, 2, (B, H, N, HD), generator=gen) * 8 - 4).double()
    perm = torch.stack([torch.stack([torch.randperm(N, generator=gen) for _ in range(H)]) for _ in range(B)])
    kk = torch.empty_like(code)
    kk.scatter_(2, perm[..., None].expand(B, H, N, HD), code)               # K[pi(i)] = s_i
    vv = torch.randn((B, H, N, HD), generator=gen)
    qkv = torch.cat([rows(code), rows(kk), rows(vv)], 1).to(BF16)
    dout = torch.randn((B * N, D), generator=gen).to(BF16)
    S = 0.125 * (code @ kk.transpose(-1, -2))
    match = torch.zeros_like(S, dtype=torch.bool).scatter_(3, perm[..., None], True)
    assert bool((S[match] == 128).all())
    return dict(qkv=qkv, dout=dout, perm=perm, max_other=float(S[~match].max()) if N > 1 else -math.inf)


# ------------------------------------------------------------------------------------------ relation loss (csrc/losses.hip, ops.RelationLossFn)
def relation_bounds(fs, ft, weight, hd_s, hd_t, u=U_BF16):
    """The gradient of one column block of the q / k / v relation loss: fs [B][N][Ds], ft [B][N][Dt] float64 holding the bf16 features,
    `weight` the upstream dL/dloss_j.  loss = sum KL(softmax(R_t) || softmax(R_s)) / B with R = F F^T / sqrt(hd), so with
    G = (softmax(R_s) - softmax(R_t)) weight / (B sqrt(hd_s)):  S = G + G^T,  dF = S F.  -> (dF, elementwise bound, S)
        |dF_kernel - dF| <= u (|S||F| + |dF|) + e32 256 |S||F| + E_249 |F|
    S is rounded to bf16 once, dF is stored as bf16, the product is an fp32 sum over 256 keys.  E_249 is the rounding the first two terms
    leave out: rel_grad_kernel (losses.hip, the line `v[e] = (expf(rs - lsi) + expf(rs - lsj) - expf(rt - lti) - expf(rt - ltj)) * up`)
    combines four fp32 exponentials of fp32 Gram entries, and where student and teacher agree (unit-scale features: both softmaxes are
    ~1 on the diagonal) they cancel to |S| << each term, so an error relative to the TERMS is not covered by u |S|.  Each term p carries the
    relative error of its argument, E_R = e32 ((D + 2)(|F||F|^T / sqrt(hd) + |R|) + 4) -- the Gram is an fp32 sum of D exact products, the
    convention of E_S in bounds(), + 4 for expf and the three additions:  E_249 = |coef| ((P_s + P_s^T) E_Rs + (P_t + P_t^T) E_Rt)."""
    B = fs.shape[0]

    def soft(f, hd):
        c = 1.0 / math.sqrt(hd)
        R = c * (f @ f.transpose(1, 2))
        P = torch.exp(R - torch.logsumexp(R, -1, keepdim=True))
        E = E32 * ((f.shape[-1] + 2) * (c * (f.abs() @ f.abs().transpose(1, 2)) + R.abs()) + 4)
        return P, E

    Ps, Es = soft(fs, hd_s)
    Pt, Et = soft(ft, hd_t)
    coef = float(weight) / (B * math.sqrt(hd_s))
    S = coef * (Ps + Ps.transpose(1, 2) - Pt - Pt.transpose(1, 2))
    E249 = abs(coef) * ((Ps + Ps.transpose(1, 2)) * Es + (Pt + Pt.transpose(1, 2)) * Et)
    dF = S @ fs
    SF = S.abs() @ fs.abs()
    return dF, u * (SF + dF.abs()) + E32 * 256 * SF + E249 @ fs.abs(), S


def relation_emulate(fs, ft, weight, hd_s, hd_t, mutate=False):
    """the launches of ops.RelationLossFn.backward in fp32 torch: fp32 Grams and log-sum-exps, line 249 in fp32, S to bf16, dF = bf16(fp32 S F).
    mutate: S = G instead of G + G^T (the transposed half of the gradient lost)."""
    B = fs.shape[0]

    def soft(f, hd):
        R = (f.to(F32) @ f.to(F32).transpose(1, 2)) * torch.tensor(1.0 / math.sqrt(hd), dtype=F32)
        return R, torch.logsumexp(R, -1)

    (rs, ls), (rt, lt) = soft(fs, hd_s), soft(ft, hd_t)
    up = torch.tensor(float(weight), dtype=F32) * torch.tensor(1.0 / (B * math.sqrt(hd_s)), dtype=F32)
    if mutate:
        S = (torch.exp(rs - ls[:, :, None]) - torch.exp(rt - lt[:, :, None])) * up
    else:
        S = (torch.exp(rs - ls[:, :, None]) + torch.exp(rs - ls[:, None, :]) - torch.exp(rt - lt[:, :, None]) - torch.exp(rt - lt[:, None, :])) * up
    return (S.to(BF16).to(F64) @ fs).to(F32).to(BF16).to(F64)


# ------------------------------------------------------------------------------------------ the shared check
def check_packed(chk, tag, qkv, B, N, H, gate, scale, out, lse, dout=None, dqkv=None, add=None, u=U_BF16, f16=False, keep=None, s=None):
    """One packed launch's outputs (2-D buffers, live rows first) against the model: O, lse and, where given, dQ / dK / dV each against
    its own bound, through chk(worst err / bound, 1.0, name=...).  -> dict name -> ratio; raises AssertionError on the first that is >= 1."""
    q, k, v, do, ad = split_packed(qkv, B, N, H, dout, add)
    ref, bnd = bounds(q, k, v, gate, scale, do, ad, u=u, f16=f16, keep=keep, s=s)
    got = dict(O=heads(out, B, N, H), lse=lse.to(F64).view(B, H, N))
    if dqkv is not None:
        D = H * HD
        got.update(dQ=heads(dqkv, B, N, H, 0), dK=heads(dqkv, B, N, H, D), dV=heads(dqkv, B, N, H, 2 * D))
    return check_outputs(chk, tag, got, ref, bnd)


def check_outputs(chk, tag, got, ref, bnd):
    res = {name: ratio(got[name], ref[name], bnd[name]) for name in got}
    print(tag, " ".join(f"{n} {x:.3f}" for n, x in res.items()))
    bad = [n for n, x in res.items() if not chk(x, 1.0, name=f"{tag}/{n}")]
    assert not bad, f"{tag}: worst |err| / bound {res}"
    return res
