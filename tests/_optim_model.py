"""Float64 statements, first-order elementwise error bounds, fp32 emulations with planted bugs, case lists and seeded inputs for the optimizer of
csrc/optim.hip: the squared gradient norm (devit_sumsq_f32) and the five fused tails -- devit_adamw_step (adamw), devit_sgd_step (momentum, nesterov),
devit_adam_l2_step (adam) and devit_lamb_step (lamb, lambc).  Plain torch on the CPU, in the conventions of tests/_tail_model.py (whose U, ratio and
gen it reuses); shared by tests/test_optim_model.py (the model under test, no GPU) and tests/test_gpu_optim.py (the kernels under test), which
therefore see the same inputs.

Every bound is u = 2^-24 times the absolute values of the terms that enter an element times the roundings on the longest path to it, counted from the
kernel's statement: a correctly rounded operation 1, sqrtf and `/` 2; a fused multiply-add only removes a rounding.  The tails share one frame, and so
do their statements: the clip (optim.hip: tail_clip -> clip64, _clip32): sqrtf 2, times grad_scale 1, + 1e-6 1, the division 2, clip *= c 1: 7;
g' = g * clip: CLIP_R = 8; the exemption from weight decay by granule (_exempt); the Adam update (_adam_update); the EMA (model_tail -> _ema)."""
import math

import torch

import _tail_model as T
from _tail_model import F32, F64, U, _f

ADAM_HP = dict(beta1=0.9, beta2=0.999, eps=1e-8, wd=0.05, ema_decay=0.999, lr=1e-3)
OPT_HP = dict(ADAM_HP, momentum=0.9)
CLIP_R = 8
CHUNK = 4096                     # elements of a LAMB chunk: 1024 granules
# outputs that are a few roundings of values of their own magnitude: the bound is a correct implementation's worst case (see _tail_model.SHORT_PATHS)
SHORT_PATHS = {"p": "the decay or the update's quotient, the subtraction", "m": "m = beta1 m + (1 - beta1) g': 3 on |beta1 m| + |m'|", "v": "as m",
               "ema": "ema = ema d + (1 - d) p: 3", "buf": "buf = mu buf + d: as m"}

ADAMW_NS = (8, 12292, 4194316)           # the sizes of step_cases
SUMSQ_NS = (4, 1024, 12292, 1048584, 4194316)
ADAMW_MUTATIONS = ("clip_without_grad_scale", "decay_on_exempt_granule", "granule_index_per_element")
SGD_MUTATIONS = ("decay_on_exempt_granule", "granule_index_per_element", "nesterov_uses_old_buf")
ADAM_MUTATIONS = ("decay_on_exempt_granule", "granule_index_per_element", "decoupled_decay")
LAMB_MUTATIONS = ("norm_over_chunk", "norm_includes_next_granule", "trust_on_no_decay_tensor", "internal_clip_forgotten", "lambc_not_capped")


# ============================================================================================ the norm (sumsq_stage1, sumsq_stage2)
def sumsq_inputs(n, ints):
    g = T.gen("sumsq", n, ints)
    return T.randint(g, -2, 2, n) if ints else T.randn(g, n) * 0.3


def sumsq_bounds(gv):
    """1024 blocks of 256 threads: per thread ceil(n / 4 / 262144) trips of a four-term expression added to s (4 products + 4 adds: 5 on the longest
    path), 6 shuffle adds and 3 through LDS (sumsq_stage1); stage 2: 4 in sequence, 6 and 3"""
    n = gv.numel()
    cnt = 5 * ((n // 4 + 262143) // 262144) + 9 + 13
    ref = (gv.to(F64) ** 2).sum()
    return ref, U * cnt * ref


# ============================================================================================ what the tails share
def step_cases():
    """the cases of devit_adamw_step, devit_sgd_step and devit_adam_l2_step: n = 8, n = 12292 (an odd number of granules, the mask alternating by
    granule) and one at n = 4194316 (the grid stride's second trip); clip active (0.05) and not (1e9), with and without gnorm_sq, EMA and the bf16
    copy, grad_scale 1 / 0.5.  dicts: n, max_norm, gnorm (gnorm_sq given), grad_scale, mask, ema, p16"""
    return [dict(n=8, max_norm=0.05, gnorm=True, grad_scale=1.0, mask=True, ema=True, p16=True),
            dict(n=8, max_norm=1e9, gnorm=True, grad_scale=0.5, mask=False, ema=False, p16=False),
            dict(n=12292, max_norm=0.05, gnorm=True, grad_scale=0.5, mask=True, ema=True, p16=True),
            dict(n=12292, max_norm=0.05, gnorm=False, grad_scale=0.5, mask=True, ema=False, p16=True),
            dict(n=12292, max_norm=1e9, gnorm=True, grad_scale=1.0, mask=False, ema=True, p16=False),
            dict(n=4194316, max_norm=0.05, gnorm=True, grad_scale=0.5, mask=True, ema=True, p16=True)]


def step_inputs(c):
    """p, three gradients (one per step; elements 0, 5 and every 7th are 0 at step 1), the no_decay4 mask alternating by granule"""
    n = c["n"]
    g = T.gen("adamw", n, c["max_norm"], c["grad_scale"])
    p = T.randn(g, n)
    grads = [T.randn(g, n) * 0.3 for _ in range(3)]
    grads[0][::7] = 0.0
    grads[0][5] = 0.0
    mask = (torch.arange(n // 4) % 2).to(torch.uint8)
    return dict(p=p, grads=grads, mask=mask if c["mask"] else None)


def _hp(hp, step):
    b1, b2, eps, wd, d, lr = (_f(hp[k]) for k in ("beta1", "beta2", "eps", "wd", "ema_decay", "lr"))
    return b1, b2, eps, wd, d, lr, _f(1 - hp["beta1"] ** step), _f(1 - hp["beta2"] ** step)


def clip64(gnorm_sq, max_norm, grad_scale):
    clip = _f(grad_scale)
    if gnorm_sq is not None:
        c = _f(max_norm) / (math.sqrt(float(gnorm_sq)) * _f(grad_scale) + _f(1e-6))
        clip = _f(grad_scale) * min(1.0, c)
    return clip


def _decayed_grad(p, g, mask, gnorm_sq, max_norm, grad_scale, wd):
    """d = g' + wd p with wd = 0 on exempt granules -> (g', d, e_d): g' 8 u; wd p 1, the add 1 on |d| (exact where wd = 0: d = g' + 0)"""
    g2 = g * clip64(gnorm_sq, max_norm, grad_scale)
    wdv = torch.full_like(p, wd) if mask is None else torch.where(mask.repeat_interleave(4).bool(), torch.zeros_like(p), torch.full_like(p, wd))
    d = g2 + wdv * p
    e_d = CLIP_R * U * g2.abs() + torch.where(wdv != 0, U * (wdv * p).abs() + U * d.abs(), torch.zeros_like(p))
    return g2, d, e_d


def _adam_update(m2, v2, e_m, e_v, lr, bc1, bc2, eps):
    """upd = ((lr / bc1) m') / (sqrtf(v') / sqrtf(bc2) + eps) -> (upd, e_upd): s = sqrtf / sqrtf: e_v / (2 v') + 2, 2, 2; + eps 1; lr / bc1 2, times
    m' 1 + e_m, the division 2 + e_denom"""
    s = v2.sqrt() / math.sqrt(bc2)
    denom = s + eps
    rel_v = torch.where(v2 > 0, e_v / (2 * v2.clamp_min(1e-300)), torch.zeros_like(v2))
    e_denom = s * (rel_v + 6 * U) + U * denom
    upd = (lr / bc1) * m2 / denom
    return upd, upd.abs() * (5 * U + e_denom / denom) + (lr / bc1) * e_m / denom


def _ema(ref, bnd, ema, d):
    if ema is not None:
        e, od = ema.to(F64), _f(1.0 - d)
        ref["ema"] = e * d + od * ref["p"]                 # ema d 1, (1 - d) p' 1 + e_p, the add 1 on |ema'|
        bnd["ema"] = U * ((e * d).abs() + (od * ref["p"]).abs()) + od * bnd["p"] + U * ref["ema"].abs()
    return ref, bnd


def _exempt(mask, n, mutate):
    if mask is None or mutate == "decay_on_exempt_granule":
        return torch.zeros(n, dtype=torch.bool)
    if mutate == "granule_index_per_element":
        return mask[torch.arange(n) % mask.numel()].bool()
    return mask.repeat_interleave(4).bool()


def _clip32(gnorm_sq, max_norm, grad_scale, norm_scaled=True):
    """tail_clip in fp32 torch; norm_scaled=False plants a bug: the norm is taken of the unscaled gradients"""
    f = lambda x: torch.tensor(x, dtype=F32)
    clip = f(grad_scale)
    if gnorm_sq is not None:
        c = f(max_norm) / (torch.sqrt(gnorm_sq.to(F32).reshape(())) * f(grad_scale if norm_scaled else 1.0) + f(1e-6))
        clip = clip * torch.minimum(c, f(1.0))
    return clip


# ============================================================================================ AdamW (adamw_kernel)
def adamw_step_bounds(p, g, m, v, ema, mask, gnorm_sq, step, max_norm, grad_scale, hp=ADAM_HP):
    """One step of the header's formula in float64 from the GIVEN fp32 state (p, m, v, ema before the step; gnorm_sq as given or None) -> (ref dict
    p, m, v, ema, bounds dict), with the hyper-parameters as the fp32 values the entry point receives (1 - beta is exact in fp32):
    m':  beta1 m 1, (1 - beta1) g' 1 + the 8 of g', the add 1 on |m'|:      u (|beta1 m| + 9 |(1 - beta1) g'|) + u |m'|
    v':  beta2 v 1, (1 - beta2) g' g' 2 + 16, the add 1:                    u (|beta2 v| + 18 |(1 - beta2) g'^2|) + u |v'|
    p':  the decay p *= (1 - lr wd): lr wd 1, 1 - 1, the product 1: 3 u |p|;  e_upd (_adam_update);  the subtraction 1 on |p'|"""
    b1, b2, eps, wd, d, lr, bc1, bc2 = _hp(hp, step)
    ob1, ob2 = _f(1.0 - b1), _f(1.0 - b2)
    p, g, m, v = (t.to(F64) for t in (p, g, m, v))
    g2 = g * clip64(gnorm_sq, max_norm, grad_scale)
    fac = 1.0 - lr * wd
    decay = torch.full_like(p, fac) if mask is None else torch.where(mask.repeat_interleave(4).bool(), torch.ones_like(p), torch.full_like(p, fac))
    m2 = b1 * m + ob1 * g2
    v2 = b2 * v + ob2 * g2 * g2
    e_m = U * ((b1 * m).abs() + (CLIP_R + 1) * (ob1 * g2).abs()) + U * m2.abs()
    e_v = U * ((b2 * v).abs() + (2 * CLIP_R + 2) * (ob2 * g2 * g2)) + U * v2.abs()
    upd, e_upd = _adam_update(m2, v2, e_m, e_v, lr, bc1, bc2, eps)
    p2 = p * decay - upd
    return _ema(dict(p=p2, m=m2, v=v2), dict(p=3 * U * p.abs() + e_upd + U * p2.abs(), m=e_m, v=e_v), ema, d)


def adamw_step_emulate(p, g, m, v, ema, mask, gnorm_sq, step, max_norm, grad_scale, hp=ADAM_HP, mutate=None):
    """fp32 torch; mutations: clip_without_grad_scale (the norm is not scaled), decay_on_exempt_granule (the mask is ignored),
    granule_index_per_element (no_decay4 is indexed by the element, not by the granule of four)"""
    assert mutate is None or mutate in ADAMW_MUTATIONS
    f = lambda x: torch.tensor(x, dtype=F32)
    b1, b2, eps, wd, d, lr = (f(hp[k]) for k in ("beta1", "beta2", "eps", "wd", "ema_decay", "lr"))
    bc1, bc2 = f(1 - hp["beta1"] ** step), f(1 - hp["beta2"] ** step)
    p, g, m, v = (t.to(F32) for t in (p, g, m, v))
    g2 = g * _clip32(gnorm_sq, max_norm, grad_scale, norm_scaled=mutate != "clip_without_grad_scale")
    pd = torch.where(_exempt(mask, p.numel(), mutate), p, p * (f(1.0) - lr * wd))
    m2 = b1 * m + (f(1.0) - b1) * g2
    v2 = b2 * v + (f(1.0) - b2) * g2 * g2
    p2 = pd - (lr / bc1) * m2 / (torch.sqrt(v2) / torch.sqrt(bc2) + eps)
    out = dict(p=p2, m=m2, v=v2)
    if ema is not None:
        out["ema"] = ema.to(F32) * d + (f(1.0) - d) * p2
    return out


# ============================================================================================ SGD with momentum (sgd_kernel)
def sgd_step_bounds(p, g, buf, ema, mask, gnorm_sq, step, max_norm, grad_scale, nesterov, hp=OPT_HP):
    """One step from the GIVEN fp32 state: d = g' + wd p; buf' = mu buf + d; p' = p - lr (nesterov ? d + mu buf' : buf') -> (ref, bounds) for p, buf, ema.
    buf': mu buf 1, + e_d, the add 1 on |buf'|.   momentum: lr buf' 1 + lr e_buf, the subtraction 1 on |p'|.
    nesterov: s = d + mu buf': e_d + mu e_buf + 1 on |mu buf'| + 1 on |s|; then lr s 1 + lr e_s, the subtraction 1."""
    wd, d_, lr, mu = _f(hp["wd"]), _f(hp["ema_decay"]), _f(hp["lr"]), _f(hp["momentum"])
    p, g, buf = (t.to(F64) for t in (p, g, buf))
    _, d, e_d = _decayed_grad(p, g, mask, gnorm_sq, max_norm, grad_scale, wd)
    buf2 = mu * buf + d
    e_buf = U * (mu * buf).abs() + e_d + U * buf2.abs()
    if nesterov:
        s = d + mu * buf2
        e_s = e_d + mu * e_buf + U * (mu * buf2).abs() + U * s.abs()
    else:
        s, e_s = buf2, e_buf
    p2 = p - lr * s
    ref, bnd = dict(p=p2, buf=buf2), dict(p=lr * e_s + U * (lr * s).abs() + U * p2.abs(), buf=e_buf)
    return _ema(ref, bnd, ema, d_)


def sgd_step_emulate(p, g, buf, ema, mask, gnorm_sq, step, max_norm, grad_scale, nesterov, hp=OPT_HP, mutate=None):
    """fp32 torch; mutations: decay_on_exempt_granule (the mask is ignored), granule_index_per_element (no_decay4 indexed by the element),
    nesterov_uses_old_buf (the look-ahead takes buf, not buf')"""
    assert mutate is None or mutate in SGD_MUTATIONS
    f = lambda x: torch.tensor(x, dtype=F32)
    wd, d_, lr, mu = (f(hp[k]) for k in ("wd", "ema_decay", "lr", "momentum"))
    p, g, buf = (t.to(F32) for t in (p, g, buf))
    g2 = g * _clip32(gnorm_sq, max_norm, grad_scale)
    d = torch.where(_exempt(mask, p.numel(), mutate), g2, g2 + wd * p)
    buf2 = mu * buf + d
    s = (d + mu * (buf if mutate == "nesterov_uses_old_buf" else buf2)) if nesterov else buf2
    out = dict(p=p - lr * s, buf=buf2)
    if ema is not None:
        out["ema"] = ema.to(F32) * d_ + (f(1.0) - d_) * out["p"]
    return out


# ============================================================================================ Adam with L2 decay (adam_l2_kernel)
def adam_step_bounds(p, g, m, v, ema, mask, gnorm_sq, step, max_norm, grad_scale, hp=OPT_HP):
    """torch.optim.Adam from the GIVEN fp32 state: d = g' + wd p; m' = b1 m + (1 - b1) d; v' = b2 v + (1 - b2) d d; p' = p - upd (no p *= 1 - lr wd).
    m': b1 m 1, (1 - b1) d 1 + e_d, the add 1 on |m'|.   v': b2 v 1, ((1 - b2) d) d 2 + 2 |d| e_d, the add 1.   p': e_upd, the subtraction 1."""
    b1, b2, eps, wd, d_, lr, bc1, bc2 = _hp(hp, step)
    ob1, ob2 = _f(1.0 - b1), _f(1.0 - b2)
    p, g, m, v = (t.to(F64) for t in (p, g, m, v))
    _, d, e_d = _decayed_grad(p, g, mask, gnorm_sq, max_norm, grad_scale, wd)
    m2 = b1 * m + ob1 * d
    v2 = b2 * v + ob2 * d * d
    e_m = U * ((b1 * m).abs() + (ob1 * d).abs()) + ob1 * e_d + U * m2.abs()
    e_v = U * ((b2 * v).abs() + 2 * ob2 * d * d) + 2 * ob2 * d.abs() * e_d + U * v2.abs()
    upd, e_upd = _adam_update(m2, v2, e_m, e_v, lr, bc1, bc2, eps)
    p2 = p - upd
    return _ema(dict(p=p2, m=m2, v=v2), dict(p=e_upd + U * p2.abs(), m=e_m, v=e_v), ema, d_)


def adam_step_emulate(p, g, m, v, ema, mask, gnorm_sq, step, max_norm, grad_scale, hp=OPT_HP, mutate=None):
    """fp32 torch; mutations: decay_on_exempt_granule, granule_index_per_element, decoupled_decay (p *= 1 - lr wd as AdamW, the gradient untouched)"""
    assert mutate is None or mutate in ADAM_MUTATIONS
    f = lambda x: torch.tensor(x, dtype=F32)
    b1, b2, eps, wd, d_, lr = (f(hp[k]) for k in ("beta1", "beta2", "eps", "wd", "ema_decay", "lr"))
    bc1, bc2 = f(1 - hp["beta1"] ** step), f(1 - hp["beta2"] ** step)
    p, g, m, v = (t.to(F32) for t in (p, g, m, v))
    g2 = g * _clip32(gnorm_sq, max_norm, grad_scale)
    exempt = _exempt(mask, p.numel(), mutate)
    if mutate == "decoupled_decay":
        d, p = g2, torch.where(exempt, p, p * (f(1.0) - lr * wd))
    else:
        d = torch.where(exempt, g2, g2 + wd * p)
    m2 = b1 * m + (f(1.0) - b1) * d
    v2 = b2 * v + (f(1.0) - b2) * d * d
    out = dict(p=p - (lr / bc1) * m2 / (torch.sqrt(v2) / torch.sqrt(bc2) + eps), m=m2, v=v2)
    if ema is not None:
        out["ema"] = ema.to(F32) * d_ + (f(1.0) - d_) * out["p"]
    return out


# ============================================================================================ LAMB (lamb_moments / lamb_trust / lamb_apply)
LAMB_SIZES = (4, 8, 4096, 4100, 12292, 12288, 8)          # one granule; two; exactly one chunk; a chunk + a granule; three chunks + a granule; three chunks
LAMB_P_SCALE = (3.0, 0.1, 0.1, 3.0, 3.0, 0.0, 0.0)        # trust above and below 1 among the decayed tensors of either parity; tensor 5: p = 0, g != 0
LAMB_GAPS = {2: 4, 5: 8}                                   # padding granules in front of tensors 2 and 5: no chunk covers them
GAP = -7.0


def lamb_cases():
    """dicts: trust_clip (lambc), exempt_parity (tensors s with s % 2 == parity are in the no-decay group; tensor 6 -- p, g, m, v all zero -- is always
    decayed), max_norm (0: no --clip-grad, LAMB's own clip alone; 0.05: the outer clip leaves norm 0.05 < 1; 5.0: both act), grad_scale, ema"""
    return [dict(trust_clip=False, exempt_parity=0, max_norm=0.0, grad_scale=1.0, ema=True),
            dict(trust_clip=False, exempt_parity=1, max_norm=5.0, grad_scale=0.5, ema=True),
            dict(trust_clip=True, exempt_parity=0, max_norm=5.0, grad_scale=0.5, ema=False),
            dict(trust_clip=True, exempt_parity=1, max_norm=0.05, grad_scale=1.0, ema=True)]


def lamb_inputs(c):
    """layout [(offset, numel, exempt)], n, p, m0, v0 (zero on tensor 6, else random: 'given state'), three gradients; the padding holds GAP in p, m, v"""
    g = T.gen("lamb", c["exempt_parity"], c["max_norm"])
    layout, off = [], 0
    for s, numel in enumerate(LAMB_SIZES):
        off += LAMB_GAPS.get(s, 0)
        layout.append((off, numel, s != 6 and s % 2 == c["exempt_parity"]))
        off += numel
    n = (off + 4 + 127) // 128 * 128
    p, m0, v0 = (torch.full((n,), GAP) for _ in range(3))
    grads = [T.randn(g, n) * 0.3 for _ in range(3)]
    for s, (o, numel, _) in enumerate(layout):
        p[o:o + numel] = T.randn(g, numel) * LAMB_P_SCALE[s]
        m0[o:o + numel] = T.randn(g, numel) * 0.01 if s != 6 else 0.0
        v0[o:o + numel] = T.randn(g, numel).abs() * 1e-4 if s != 6 else 0.0
        if s == 6:
            for gr in grads:
                gr[o:o + numel] = 0.0
    grads[0][::7] = 0.0
    return dict(layout=layout, n=n, p=p, m=m0, v=v0, grads=grads)


def lamb_sum_roundings(numel):
    """roundings of a tensor's sum of squares: per thread <= 4 trips of a four-term expression added to s (5 each; lamb_moments_kernel), 6 shuffle adds
    and 3 through LDS; lamb_trust_kernel: ceil(chunks / 64) adds per lane, 6 shuffle adds"""
    chunks = (numel + CHUNK - 1) // CHUNK
    return 5 * 4 + 9 + (chunks + 63) // 64 + 6


def lamb_step_bounds(p, g, m, v, ema, layout, gnorm_sq, step, max_norm, grad_scale, trust_clip, hp=OPT_HP):
    """timm Lamb from the GIVEN fp32 state -> (ref, bounds) for p, m, v, ema over the flat buffer (elements of no tensor: unchanged, bound 0) and trust
    [len(layout)].  max_norm <= 0: no outer clip.
    c2 = clip / max(1, n1), n1 = sqrtf(gnorm_sq) clip: clip 7, n1 2 + 1 + 7 = 10, the division 2: 19; g'' = g c2: RG = 20
    m', v' as adamw_step_bounds from g'' (RG + 1, 2 RG + 2).   u0 = (m' / bc1) / (sqrtf(v') / sqrtf(bc2) + eps): m' / bc1 2 + e_m / bc1; the denominator as
    _adam_update; the division 2.   u = u0 + wd p: 1 on |wd p|, 1 on |u| (decayed tensors).
    sum p^2, sum u^2: lamb_sum_roundings, + 2 |u| e_u per term; sqrtf 2 each, the division 2 -> e_trust.
    p' = p - (lr trust) u: e_trust |lr u| + lr trust e_u, lr trust 1, the product 1, the subtraction 1 on |p'|"""
    b1, b2, eps, wd, d_, lr, bc1, bc2 = _hp(hp, step)
    ob1, ob2 = _f(1.0 - b1), _f(1.0 - b2)
    p, g, m, v = (t.to(F64) for t in (p, g, m, v))
    clip = clip64(gnorm_sq if max_norm > 0 else None, max_norm, grad_scale)
    n1 = math.sqrt(float(gnorm_sq)) * clip
    g2 = g * (clip / max(1.0, n1))
    RG = 20
    m2 = b1 * m + ob1 * g2
    v2 = b2 * v + ob2 * g2 * g2
    e_m = U * ((b1 * m).abs() + (RG + 1) * (ob1 * g2).abs()) + U * m2.abs()
    e_v = U * ((b2 * v).abs() + (2 * RG + 2) * (ob2 * g2 * g2)) + U * v2.abs()
    s = v2.clamp_min(0).sqrt() / math.sqrt(bc2)
    denom = s + eps
    rel_v = torch.where(v2 > 0, e_v / (2 * v2.clamp_min(1e-300)), torch.zeros_like(v2))
    e_denom = s * (rel_v + 6 * U) + U * denom
    mh = m2 / bc1
    u0 = mh / denom
    e_u0 = (e_m / bc1 + 2 * U * mh.abs()) / denom + u0.abs() * e_denom / denom + 2 * U * u0.abs()
    ref = dict(p=p.clone(), m=m.clone(), v=v.clone(), trust=torch.ones(len(layout), dtype=F64))
    bnd = dict(p=torch.zeros_like(p), m=torch.zeros_like(p), v=torch.zeros_like(p), trust=torch.zeros(len(layout), dtype=F64))
    for si, (o, numel, exempt) in enumerate(layout):
        sl = slice(o, o + numel)
        ref["m"][sl], ref["v"][sl], bnd["m"][sl], bnd["v"][sl] = m2[sl], v2[sl], e_m[sl], e_v[sl]
        ps = p[sl]
        if exempt:
            u, e_u, trust, e_t = u0[sl], e_u0[sl], 1.0, 0.0
        else:
            u = u0[sl] + wd * ps
            e_u = e_u0[sl] + U * (wd * ps).abs() + U * u.abs()
            sp, su, cnt = float((ps * ps).sum()), float((u * u).sum()), lamb_sum_roundings(numel)
            trust, e_t = 1.0, 0.0
            if sp > 0 and su > 0:
                e_su = cnt * U * su + 2 * float((u.abs() * e_u).sum())
                trust = math.sqrt(sp) / math.sqrt(su)
                e_t = trust * (cnt * U / 2 + 2 * U + e_su / (2 * su) + 2 * U + 2 * U)
            if trust_clip:
                trust = min(trust, 1.0)
        upd = lr * trust * u
        ref["p"][sl] = ps - upd
        bnd["p"][sl] = e_t * (lr * u).abs() + lr * trust * e_u + 2 * U * upd.abs() + U * ref["p"][sl].abs()
        ref["trust"][si], bnd["trust"][si] = trust, e_t
    if ema is not None:
        e, od = ema.to(F64), _f(1.0 - d_)
        ref["ema"], bnd["ema"] = e.clone(), torch.zeros_like(p)
        for o, numel, _ in layout:
            sl = slice(o, o + numel)
            ref["ema"][sl] = e[sl] * d_ + od * ref["p"][sl]
            bnd["ema"][sl] = U * ((e[sl] * d_).abs() + (od * ref["p"][sl]).abs()) + od * bnd["p"][sl] + U * ref["ema"][sl].abs()
    return ref, bnd


def lamb_step_emulate(p, g, m, v, ema, layout, gnorm_sq, step, max_norm, grad_scale, trust_clip, hp=OPT_HP, mutate=None):
    """fp32 torch, tensor by tensor (torch's own summation order); mutations: norm_over_chunk (each 4096-element chunk takes the ratio of its own
    norms), norm_includes_next_granule (the norms run four elements past the tensor's end), trust_on_no_decay_tensor (always_adapt on),
    internal_clip_forgotten (timm Lamb's max_grad_norm = 1 left out), lambc_not_capped.  trust is the first chunk's under norm_over_chunk."""
    assert mutate is None or mutate in LAMB_MUTATIONS
    f = lambda x: torch.tensor(x, dtype=F32)
    b1, b2, eps, wd, d_, lr = (f(hp[k]) for k in ("beta1", "beta2", "eps", "wd", "ema_decay", "lr"))
    bc1, bc2 = f(1 - hp["beta1"] ** step), f(1 - hp["beta2"] ** step)
    p, g, m, v = (t.to(F32) for t in (p, g, m, v))
    clip = _clip32(gnorm_sq if max_norm > 0 else None, max_norm, grad_scale)
    n1 = torch.sqrt(gnorm_sq.to(F32).reshape(())) * clip
    if n1 > 1 and mutate != "internal_clip_forgotten":
        clip = clip / n1
    g2 = g * clip
    out = dict(p=p.clone(), m=m.clone(), v=v.clone(), trust=torch.ones(len(layout)))
    if ema is not None:
        out["ema"] = ema.to(F32).clone()

    def ratio_of(ps, us):
        wn, un = torch.sqrt((ps * ps).sum()), torch.sqrt((us * us).sum())
        t = wn / un if (wn > 0 and un > 0) else f(1.0)
        return torch.minimum(t, f(1.0)) if (trust_clip and mutate != "lambc_not_capped") else t

    for si, (o, numel, exempt) in enumerate(layout):
        sl = slice(o, o + numel)
        m2 = b1 * m[sl] + (f(1.0) - b1) * g2[sl]
        v2 = b2 * v[sl] + (f(1.0) - b2) * g2[sl] * g2[sl]
        u = (m2 / bc1) / (torch.sqrt(v2) / torch.sqrt(bc2) + eps)
        if not exempt:
            u = u + wd * p[sl]
        trust = torch.ones(numel)
        if not exempt or mutate == "trust_on_no_decay_tensor":
            if mutate == "norm_over_chunk":
                for c0 in range(0, numel, CHUNK):
                    trust[c0:c0 + CHUNK] = ratio_of(p[sl][c0:c0 + CHUNK], u[c0:c0 + CHUNK])
            elif mutate == "norm_includes_next_granule":
                ext = slice(o, o + numel + 4)
                m2e = b1 * m[ext] + (f(1.0) - b1) * g2[ext]
                v2e = b2 * v[ext] + (f(1.0) - b2) * g2[ext] * g2[ext]
                ue = (m2e / bc1) / (torch.sqrt(v2e.abs()) / torch.sqrt(bc2) + eps) + wd * p[ext]
                trust[:] = ratio_of(p[ext], ue)
            else:
                trust[:] = ratio_of(p[sl], u)
        out["m"][sl], out["v"][sl] = m2, v2
        out["p"][sl] = p[sl] - (lr * trust) * u
        out["trust"][si] = trust[0]
        if ema is not None:
            out["ema"][sl] = out["ema"][sl] * d_ + (f(1.0) - d_) * out["p"][sl]
    return out


def lamb_naive(p, g, m, v, layout, gnorm_sq, step, max_norm, grad_scale, trust_clip, hp=OPT_HP):
    """timm Lamb.step written as its loop over parameter tensors, in float64 python / torch, for one step from the given state: the second
    statement lamb_step_bounds' reference is checked against (tests/test_optim_model.py)"""
    b1, b2, eps, wd, _, lr, bc1, bc2 = _hp(hp, step)
    p, g, m, v = (t.to(F64).clone() for t in (p, g, m, v))
    scale = _f(grad_scale)
    if max_norm > 0:                                                   # NativeScaler: clip_grad_norm_ over the true (scaled) gradients
        scale *= min(1.0, _f(max_norm) / (math.sqrt(float(gnorm_sq)) * _f(grad_scale) + _f(1e-6)))
    grads = [g[o:o + n_] * scale for o, n_, _ in layout]
    global_norm = math.sqrt(float(gnorm_sq)) * scale                   # the norm over the whole buffer, as the optimizer sees it
    clip_global = global_norm / 1.0 if global_norm > 1.0 else 1.0      # max_grad_norm = 1.0
    trusts = []
    for (o, n_, exempt), grad in zip(layout, grads):
        grad = grad / clip_global
        exp_avg = m[o:o + n_].mul_(b1).add_(grad, alpha=1 - b1)        # grad_averaging: beta3 = 1 - beta1 (taken in fp32, as the kernel's 1 - beta1)
        exp_avg_sq = v[o:o + n_].mul_(b2).addcmul_(grad, grad, value=1 - b2)
        update = (exp_avg / bc1) / ((exp_avg_sq.sqrt() / math.sqrt(bc2)) + eps)
        group_wd = 0.0 if exempt else wd
        if group_wd != 0:
            update = update + group_wd * p[o:o + n_]
        trust = 1.0
        if group_wd != 0:                                              # always_adapt is off
            w_norm, g_norm = float(p[o:o + n_].norm(2.0)), float(update.norm(2.0))
            trust = w_norm / g_norm if (w_norm > 0 and g_norm > 0) else 1.0
            if trust_clip:
                trust = min(trust, 1.0)
        p[o:o + n_] -= lr * trust * update
        trusts.append(trust)
    return dict(p=p, m=m, v=v, trust=torch.tensor(trusts, dtype=F64))
