"""The model of the fused tails with a learning rate per granule (csrc/optim.hip: adamw_lrs_kernel, sgd_lrs_kernel, adam_l2_lrs_kernel,
lamb_apply_lrs_kernel; devit_*_step_lrs): the float64 statements, elementwise bounds and fp32 emulations of tests/_optim_model.py, called once per
group with the learning rate replaced by the granule's, lr_g = fp32(fp32(lr) * fp32(scale_g)) -- the one fp32 multiply the kernels make.  lr_g is an
exact fp32 value and stands in the kernels wherever lr stands in their siblings, so every bound of _optim_model holds unchanged with lr_g as the
given learning rate; an element takes the result of its granule's group.  Nothing of _optim_model is edited.  Shared by tests/test_lrscale_model.py
(the model under test, no GPU) and tests/test_gpu_lrscale.py (the kernels), which see the same cases and inputs.

Three planted bugs (MUTATIONS), each of which the bounds must catch: group_index_per_element (lr_group4 indexed by the element, not by the
granule of four), adamw_decay_on_base_lr (p *= 1 - lr wd with the unscaled lr, the update scaled), lamb_scale_in_trust_norm (the trust ratio is
||p|| / ||scale u||: the scale enters the norm and cancels itself in lr scale trust u)."""
import torch

import _optim_model as M
from _tail_model import F32, F64

TABLE = 256
MUTATIONS = ("group_index_per_element", "adamw_decay_on_base_lr", "lamb_scale_in_trust_norm")
KINDS = ("adamw", "adam", "momentum", "nesterov")


def lr_of(hp, scale):
    """fp32(lr) * fp32(scale) rounded to fp32, as a python float"""
    return float(torch.tensor(hp["lr"], dtype=F32) * torch.tensor(scale, dtype=F32))


def element_groups(group4, mutate=None):
    """the group byte of every element: its granule's (the bug: the byte array indexed by the element)"""
    n = group4.numel() * 4
    if mutate == "group_index_per_element":
        return group4[torch.arange(n) % group4.numel()].long()
    return group4.long().repeat_interleave(4)


def _per_group(fn, group4, table, hp, mutate=None):
    """fn(hp with the group's lr) -> dict of [n] tensors, or a tuple of such dicts; every element from the call of its granule's group"""
    grp = element_groups(group4, mutate)
    out = None
    for b in sorted(set(grp.tolist())):
        res = fn(dict(hp, lr=lr_of(hp, float(table[b]))))
        res = res if isinstance(res, tuple) else (res,)
        if out is None:
            out = tuple({k: v.clone() for k, v in d.items()} for d in res)
        sel = grp == b
        for o, d in zip(out, res):
            for k in d:
                o[k][sel] = d[k][sel]
    return out if len(out) > 1 else out[0]


# ============================================================================================ AdamW, SGD, Adam
def step_bounds(kind, group4, table, p, g, state, ema, mask, gnorm_sq, step, max_norm, grad_scale, hp=None):
    """(ref, bounds) of one step of `kind` (KINDS) from the given fp32 state (state: (m, v), or (buf,) for momentum / nesterov)"""
    hp = hp or (M.ADAM_HP if kind == "adamw" else M.OPT_HP)
    tail = (ema, mask, gnorm_sq, step, max_norm, grad_scale)
    if kind == "adamw":
        fn = lambda h: M.adamw_step_bounds(p, g, *state, *tail, hp=h)
    elif kind == "adam":
        fn = lambda h: M.adam_step_bounds(p, g, *state, *tail, hp=h)
    else:
        fn = lambda h: M.sgd_step_bounds(p, g, *state, *tail, kind == "nesterov", hp=h)
    return _per_group(fn, group4, table, hp)


def _adamw_decay_on_base_lr(group4, table, p, g, m, v, ema, mask, gnorm_sq, step, max_norm, grad_scale, hp):
    """adamw_step_emulate's lines with two learning rates: the base lr in the decay, the granule's in the update"""
    f = lambda x: torch.tensor(x, dtype=F32)
    b1, b2, eps, wd, d, lr0 = (f(hp[k]) for k in ("beta1", "beta2", "eps", "wd", "ema_decay", "lr"))
    bc1, bc2 = f(1 - hp["beta1"] ** step), f(1 - hp["beta2"] ** step)
    lr = lr0 * table.to(F32)[element_groups(group4)]
    p, g, m, v = (t.to(F32) for t in (p, g, m, v))
    g2 = g * M._clip32(gnorm_sq, max_norm, grad_scale)
    pd = torch.where(M._exempt(mask, p.numel(), None), p, p * (f(1.0) - lr0 * wd))
    m2 = b1 * m + (f(1.0) - b1) * g2
    v2 = b2 * v + (f(1.0) - b2) * g2 * g2
    out = dict(p=pd - (lr / bc1) * m2 / (torch.sqrt(v2) / torch.sqrt(bc2) + eps), m=m2, v=v2)
    if ema is not None:
        out["ema"] = ema.to(F32) * d + (f(1.0) - d) * out["p"]
    return out


def step_emulate(kind, group4, table, p, g, state, ema, mask, gnorm_sq, step, max_norm, grad_scale, hp=None, mutate=None):
    """fp32 torch: _optim_model's emulation per group; mutations group_index_per_element, adamw_decay_on_base_lr (AdamW only)"""
    assert mutate is None or mutate in MUTATIONS[:2]
    hp = hp or (M.ADAM_HP if kind == "adamw" else M.OPT_HP)
    tail = (ema, mask, gnorm_sq, step, max_norm, grad_scale)
    if mutate == "adamw_decay_on_base_lr":
        assert kind == "adamw"
        return _adamw_decay_on_base_lr(group4, table, p, g, *state, *tail, hp)
    if kind == "adamw":
        fn = lambda h: M.adamw_step_emulate(p, g, *state, *tail, hp=h)
    elif kind == "adam":
        fn = lambda h: M.adam_step_emulate(p, g, *state, *tail, hp=h)
    else:
        fn = lambda h: M.sgd_step_emulate(p, g, *state, *tail, kind == "nesterov", hp=h)
    return _per_group(fn, group4, table, hp, mutate)


def step_cases():
    """the cases of the three grid-stride tails: _optim_model.step_cases' keys plus cuts (the granules at which a new group starts: none a multiple
    of 64), bytes (the group's byte in lr_group4) and scales (its table entry; the rest of the table holds NaN where the test wants to see that no
    other entry is read, 1.0 otherwise).  n = 8: two granules in two groups; n = 12292 (3073 granules): four groups with a scale of 0 under byte 255,
    and 26 groups (a 24-block model's)"""
    cuts26 = [0] + [118 * k + 5 for k in range(1, 26)]
    return [dict(n=8, max_norm=0.05, gnorm=True, grad_scale=1.0, mask=True, ema=True, p16=True, cuts=[0, 1], bytes=[255, 3], scales=[0.25, 0.0]),
            dict(n=12292, max_norm=0.05, gnorm=True, grad_scale=0.5, mask=True, ema=True, p16=True, cuts=[0, 37, 1001, 2050],
                 bytes=[0, 255, 7, 128], scales=[1.0, 0.0, 0.75, 0.421875]),
            dict(n=12292, max_norm=1e9, gnorm=False, grad_scale=1.0, mask=False, ema=False, p16=False, cuts=cuts26,
                 bytes=[9 * k + 3 for k in range(25)] + [255], scales=[0.75 ** (25 - k) for k in range(26)])]


def case_id(c):
    return f"n{c['n']}-g{len(c['cuts'])}-mn{c['max_norm']}-gn{int(c['gnorm'])}-e{int(c['ema'])}-mask{int(c['mask'])}"


def group_arrays(c, fill=1.0):
    """(lr_group4 [n / 4] uint8, lr_scales [256] fp32 with `fill` in the entries no group uses) of a case"""
    n4 = c["n"] // 4
    group4, table = torch.zeros(n4, dtype=torch.uint8), torch.full((TABLE,), fill, dtype=F32)
    for lo, hi, b, s in zip(c["cuts"], c["cuts"][1:] + [n4], c["bytes"], c["scales"]):
        assert 0 <= lo < hi <= n4 and (lo == 0 or lo % 64)
        group4[lo:hi] = b
        table[b] = s
    return group4, table


# ============================================================================================ LAMB
LAMB_BYTES = (0, 9, 1, 255, 2, 77, 200)                    # one group per tensor of _optim_model.LAMB_SIZES
LAMB_SCALES = (1.0, 0.5, 0.75, 0.0, 0.25, 0.125, 2.0)      # tensors 1 and 2 (trust below 1, decayed under either parity) at scales that are not 1


def lamb_group_arrays(layout, n, fill=1.0):
    """one group per tensor; the padding between tensors keeps byte 0, which is scale 1"""
    group4, table = torch.zeros(n // 4, dtype=torch.uint8), torch.full((TABLE,), fill, dtype=F32)
    table[0] = 1.0
    for (o, numel, _), b, s in zip(layout, LAMB_BYTES, LAMB_SCALES):
        group4[o // 4:(o + numel + 3) // 4] = b
        table[b] = s
    return group4, table


def _lamb_per_tensor(fn, layout, table_scales, hp):
    """fn(hp) -> dict over the flat buffer (+ trust per tensor) or a tuple of them; every tensor's elements from the call with ITS lr, the trust
    ratios from the first call (they do not see the learning rate)"""
    out = None
    for s in sorted(set(table_scales)):
        res = fn(dict(hp, lr=lr_of(hp, s)))
        res = res if isinstance(res, tuple) else (res,)
        if out is None:
            out = tuple({k: v.clone() for k, v in d.items()} for d in res)
        for (o, numel, _), st in zip(layout, table_scales):
            if st == s:
                for od, d in zip(out, res):
                    for k in d:
                        if k != "trust":
                            od[k][o:o + numel] = d[k][o:o + numel]
    return out if len(out) > 1 else out[0]


def lamb_step_bounds(scales, p, g, m, v, ema, layout, gnorm_sq, step, max_norm, grad_scale, trust_clip, hp=M.OPT_HP):
    """(ref, bounds) with tensor s of the layout at scales[s]: p' = p - (lr scale) trust u; m', v' and trust are the unscaled statement's"""
    return _lamb_per_tensor(lambda h: M.lamb_step_bounds(p, g, m, v, ema, layout, gnorm_sq, step, max_norm, grad_scale, trust_clip, hp=h),
                            layout, list(scales), hp)


def lamb_step_emulate(scales, p, g, m, v, ema, layout, gnorm_sq, step, max_norm, grad_scale, trust_clip, hp=M.OPT_HP, mutate=None):
    """fp32 torch: _optim_model's emulation per scale.  lamb_scale_in_trust_norm: p' and ema' of the decayed tensors are formed again from the
    emulation's m', v' with trust = ||p|| / ||scale u|| (1 where a norm is 0), as a kernel that scaled u in front of the norms would"""
    assert mutate is None or mutate == "lamb_scale_in_trust_norm"
    out = _lamb_per_tensor(lambda h: M.lamb_step_emulate(p, g, m, v, ema, layout, gnorm_sq, step, max_norm, grad_scale, trust_clip, hp=h),
                           layout, list(scales), hp)
    if mutate is None:
        return out
    f = lambda x: torch.tensor(x, dtype=F32)
    eps, wd, d_ = (f(hp[k]) for k in ("eps", "wd", "ema_decay"))
    bc1, bc2 = f(1 - hp["beta1"] ** step), f(1 - hp["beta2"] ** step)
    p32 = p.to(F32)
    for si, ((o, numel, exempt), s) in enumerate(zip(layout, scales)):
        if exempt:
            continue
        sl = slice(o, o + numel)
        u = (out["m"][sl] / bc1) / (torch.sqrt(out["v"][sl]) / torch.sqrt(bc2) + eps) + wd * p32[sl]
        su = f(s) * u
        wn, un = torch.sqrt((p32[sl] * p32[sl]).sum()), torch.sqrt((su * su).sum())
        t = wn / un if (wn > 0 and un > 0) else f(1.0)
        if trust_clip:
            t = torch.minimum(t, f(1.0))
        out["p"][sl] = p32[sl] - (f(lr_of(hp, s)) * t) * u
        out["trust"][si] = t
        if ema is not None:
            out["ema"][sl] = ema.to(F32)[sl] * d_ + (f(1.0) - d_) * out["p"][sl]
    return out
