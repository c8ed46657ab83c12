"""tests/_lrscale_model.py held to itself, no GPU: the fp32 emulation of every scaled tail lies within the bounds of its float64 statement on the
cases and inputs tests/test_gpu_lrscale.py gives the kernels (three chained steps), an all-ones table reproduces _optim_model's emulation bit for
bit, and each of the three planted bugs leaves the bounds."""
import pytest
import torch

import _lrscale_model as S
import _optim_model as M
from _tail_model import ratio


def _gnorm(c, g):
    return (g.double() ** 2).sum().float().reshape(1) if c["gnorm"] else None


def _chain(kind, c, mutate=None, ones=False):
    """three chained steps of the emulation, each held against the statement applied to the state it started from -> worst ratio per output"""
    i = M.step_inputs(c)
    group4, table = S.group_arrays(c)
    if ones:
        table = torch.ones_like(table)
    n = c["n"]
    state = (torch.zeros(n),) if kind in ("momentum", "nesterov") else (torch.zeros(n), torch.zeros(n))
    p, ema = i["p"], i["p"].clone() if c["ema"] else None
    worst, outs = {}, []
    for step in (1, 2, 3):
        g = i["grads"][step - 1]
        tail = (ema, i["mask"], _gnorm(c, g), step, c["max_norm"], c["grad_scale"])
        ref, bnd = S.step_bounds(kind, group4, table, p, g, state, *tail)
        got = S.step_emulate(kind, group4, table, p, g, state, *tail, mutate=mutate)
        assert set(got) == set(ref)
        for k in ref:
            worst[k] = max(worst.get(k, 0.0), ratio(got[k], ref[k], bnd[k]))
        p, ema = got["p"], got.get("ema")
        state = (got["buf"],) if "buf" in got else (got["m"], got["v"])
        outs.append(got)
    return worst, outs


@pytest.mark.parametrize("kind", S.KINDS)
@pytest.mark.parametrize("c", S.step_cases(), ids=S.case_id)
def test_emulation_within_bounds(kind, c):
    worst, _ = _chain(kind, c)
    assert all(r <= 1.0 for r in worst.values()), worst
    assert worst["p"] > 0.0, "fp32 against float64: some rounding shows"


@pytest.mark.parametrize("kind", S.KINDS)
def test_ones_table_is_the_unscaled_emulation(kind):
    c = S.step_cases()[1]
    i = M.step_inputs(c)
    _, outs = _chain(kind, c, ones=True)
    n = c["n"]
    g = i["grads"][0]
    tail = (i["p"].clone(), i["mask"], _gnorm(c, g), 1, c["max_norm"], c["grad_scale"])
    if kind == "adamw":
        want = M.adamw_step_emulate(i["p"], g, torch.zeros(n), torch.zeros(n), *tail)
    elif kind == "adam":
        want = M.adam_step_emulate(i["p"], g, torch.zeros(n), torch.zeros(n), *tail)
    else:
        want = M.sgd_step_emulate(i["p"], g, torch.zeros(n), *tail, kind == "nesterov")
    assert all(torch.equal(outs[0][k], want[k]) for k in want)


def test_scales_reach_the_parameters():
    """the statement itself: after one AdamW step without weight decay from zero moments, the group of scale 0 has not moved and the others moved by
    their scale times the plain step (float64: to 1e-6 relative, the fp32 rounding of lr scale)"""
    c = S.step_cases()[1]
    i = M.step_inputs(c)
    group4, table = S.group_arrays(c)
    n = c["n"]
    hp = dict(M.ADAM_HP, wd=0.0)
    z = torch.zeros(n)
    args = (i["p"], i["grads"][0], (z, z), None, None, None, 1, c["max_norm"], c["grad_scale"])
    ref, _ = S.step_bounds("adamw", group4, table, *args, hp=hp)
    plain, _ = S.step_bounds("adamw", group4, torch.ones_like(table), *args, hp=hp)
    scale = table.double()[S.element_groups(group4)]
    dp, dplain = ref["p"] - i["p"].double(), plain["p"] - i["p"].double()
    assert bool((dp[scale == 0] == 0).all()) and int((scale == 0).sum()) == 4 * (1001 - 37)
    assert float(((dp - scale * dplain).abs() / dplain.abs().clamp_min(1e-30)).max()) < 1e-6 and float(dplain.abs().max()) > 0


# ------------------------------------------------------------------------------------------ the planted bugs
@pytest.mark.parametrize("kind", S.KINDS)
@pytest.mark.parametrize("c", S.step_cases(), ids=S.case_id)
def test_group_index_per_element_is_caught(kind, c):
    worst, _ = _chain(kind, c, mutate="group_index_per_element")
    assert worst["p"] > 1.0, worst


@pytest.mark.parametrize("c", S.step_cases(), ids=S.case_id)
def test_adamw_decay_on_base_lr_is_caught(c):
    worst, _ = _chain("adamw", c, mutate="adamw_decay_on_base_lr")
    assert worst["p"] > 1.0, worst


# ------------------------------------------------------------------------------------------ LAMB
def _lamb_chain(c, mutate=None):
    i = M.lamb_inputs(c)
    p, m, v, ema = i["p"], i["m"], i["v"], i["p"].clone() if c["ema"] else None
    worst, trusts = {}, []
    for step in (1, 2, 3):
        g = i["grads"][step - 1]
        gsq = (g.double() ** 2).sum().float().reshape(1)
        tail = (i["layout"], gsq, step, c["max_norm"], c["grad_scale"], c["trust_clip"])
        ref, bnd = S.lamb_step_bounds(S.LAMB_SCALES, p, g, m, v, ema, *tail)
        got = S.lamb_step_emulate(S.LAMB_SCALES, p, g, m, v, ema, *tail, mutate=mutate)
        plain, _ = M.lamb_step_bounds(p, g, m, v, ema, *tail)
        assert torch.equal(ref["trust"], plain["trust"]) and torch.equal(ref["m"], plain["m"]) and torch.equal(ref["v"], plain["v"])
        for (o, numel, _), s in zip(i["layout"], S.LAMB_SCALES):          # the statement: tensor s moves by its scale times the plain step
            dp, dplain = ref["p"][o:o + numel] - p[o:o + numel].double(), plain["p"][o:o + numel] - p[o:o + numel].double()
            assert float((dp - s * dplain).abs().max()) <= 1e-6 * float(dplain.abs().max())
        for k in ref:
            worst[k] = max(worst.get(k, 0.0), ratio(got[k], ref[k], bnd[k]))
        p, m, v, ema = got["p"], got["m"], got["v"], got.get("ema")
        trusts.append(got["trust"])
    return worst


@pytest.mark.parametrize("c", M.lamb_cases(), ids=lambda c: f"clip{int(c['trust_clip'])}-par{c['exempt_parity']}-mn{c['max_norm']}")
def test_lamb_emulation_and_its_planted_bug(c):
    worst = _lamb_chain(c)
    assert all(r <= 1.0 for r in worst.values()), worst
    bad = _lamb_chain(c, mutate="lamb_scale_in_trust_norm")
    assert bad["p"] > 1.0 and bad["trust"] > 1.0, bad
