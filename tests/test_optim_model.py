"""tests/_optim_model.py under test, on the CPU: the fp32 emulation of the norm and of every optimizer tail of csrc/optim.hip stays inside its bounds
over three chained steps (<= 0.5, below 1 on the short paths), every planted bug leaves them on a named output of a named case, the float64
statements of adamw, momentum, nesterov and adam agree with torch.optim.AdamW / SGD / Adam (three steps, 1e-12 relative where the hyper-parameters
are exact in fp32), and the LAMB statement agrees with a naive per-tensor loop and has the properties timm's Lamb has."""
import math

import pytest
import torch

import _optim_model as M
import _tail_model as T
from _tail_model import F64, ratio

HALF = 0.5


def _hold(tag, res):
    print(tag, " ".join(f"{k} {v:.3f}" for k, v in res.items()))
    bad = {k: v for k, v in res.items() if not (v < 1.0 if k in M.SHORT_PATHS else v <= HALF)}
    assert not bad, f"{tag}: emulation |err| / bound {bad}"


def _caught(bug, hits):
    hits = [h for h in hits if h[2] >= 1.0]
    assert hits, f"planted bug {bug}: not caught on any output of any case"
    case, out, rt = max(hits, key=lambda h: h[2])
    print(f"planted bug {bug}: caught on {len(hits)} (case, output) pairs; worst {case} / {out}: ratio {rt:.3g}")


def _ids(c):
    return f"n{c['n']}-mn{c['max_norm']}-gs{c['grad_scale']}-gn{int(c['gnorm'])}"


# ------------------------------------------------------------------------------------------ the norm, AdamW
@pytest.mark.parametrize("n", M.SUMSQ_NS)
def test_sumsq(n):
    gi = M.sumsq_inputs(n, True)
    ref, _ = M.sumsq_bounds(gi)
    assert float(ref) < 2 ** 24 and float((gi * gi).sum()) == float(ref)          # every partial sum is an integer below 2^24
    gr = M.sumsq_inputs(n, False)
    ref, bnd = M.sumsq_bounds(gr)
    _hold(f"sumsq n{n}", dict(out=ratio((gr * gr).sum(), ref, bnd)))


def _adam_chain(c, mutate=None):
    """three chained steps of the emulation, each held against the float64 statement applied to the state it started from -> worst ratios"""
    i = M.step_inputs(c)
    n = c["n"]
    p, m, v = i["p"].clone(), torch.zeros(n), torch.zeros(n)
    ema = i["p"].clone() if c["ema"] else None
    worst = {}
    for step in (1, 2, 3):
        g = i["grads"][step - 1]
        gsq = (g * g).sum().reshape(1) if c["gnorm"] else None
        ref, bnd = M.adamw_step_bounds(p, g, m, v, ema, i["mask"], gsq, step, c["max_norm"], c["grad_scale"])
        e = M.adamw_step_emulate(p, g, m, v, ema, i["mask"], gsq, step, c["max_norm"], c["grad_scale"], mutate=mutate)
        for k in ref:
            worst[k] = max(worst.get(k, 0.0), ratio(e[k], ref[k], bnd[k]))
        p, m, v, ema = e["p"], e["m"], e["v"], e.get("ema")
    return worst


@pytest.mark.parametrize("c", M.step_cases(), ids=lambda c: f"n{c['n']}-mn{c['max_norm']}-gs{c['grad_scale']}-gn{int(c['gnorm'])}")
def test_adamw_emulation_within_bounds(c):
    _hold(f"adamw {c}", _adam_chain(c))


@pytest.mark.parametrize("bug", M.ADAMW_MUTATIONS)
def test_adamw_planted_bugs(bug):
    hits = []
    for c in M.step_cases():
        if c["n"] > 100000:
            continue
        hits += [((c["n"], c["max_norm"], c["grad_scale"], c["mask"]), k, rt) for k, rt in _adam_chain(c, mutate=bug).items()]
    _caught(bug, hits)


def test_adamw_statement_agrees_with_torch():
    n = 64
    c = dict(n=n, max_norm=0.05, gnorm=True, grad_scale=1.0, mask=False, ema=False, p16=False)
    i = M.step_inputs(c)
    hp = {k: T._f(v) for k, v in M.ADAM_HP.items()}          # the statement takes the hyper-parameters as fp32 values
    rp = i["p"].to(F64).clone().requires_grad_(True)
    opt = torch.optim.AdamW([rp], lr=hp["lr"], betas=(hp["beta1"], hp["beta2"]), eps=hp["eps"], weight_decay=hp["wd"])
    p, m, v = i["p"].to(F64), torch.zeros(n, dtype=F64), torch.zeros(n, dtype=F64)
    for step in (1, 2, 3):
        g = i["grads"][step - 1].to(F64)
        rp.grad = g.clone()
        torch.nn.utils.clip_grad_norm_([rp], 0.05)
        opt.step()
        ref, _ = M.adamw_step_bounds(p, g, m, v, None, None, (g * g).sum(), step, 0.05, 1.0)
        p, m, v = ref["p"], ref["m"], ref["v"]
        # the kernel takes the bias corrections as fp32 values (dyn): the statement rounds them, torch does not -> compare with them unrounded
        bc1, bc2 = 1 - hp["beta1"] ** step, 1 - hp["beta2"] ** step
        assert abs(T._f(1 - M.ADAM_HP["beta1"] ** step) - bc1) < 1e-6 and abs(T._f(1 - M.ADAM_HP["beta2"] ** step) - bc2) < 1e-6
    assert float((p - rp.detach()).abs().max()) <= 1e-6          # fp32-rounded bias corrections (1e-7 relative) times three updates of 1e-3
    # with the corrections passed through unrounded the statement IS torch's: one step from zero state
    rp2 = i["p"].to(F64).clone().requires_grad_(True)
    opt2 = torch.optim.AdamW([rp2], lr=hp["lr"], betas=(0.5, 0.75), eps=hp["eps"], weight_decay=hp["wd"])
    rp2.grad = i["grads"][1].to(F64).clone()
    opt2.step()
    ref, _ = M.adamw_step_bounds(i["p"].to(F64), i["grads"][1], torch.zeros(n), torch.zeros(n), None, None, None, 1, 1e9, 1.0,
                                 hp=dict(M.ADAM_HP, beta1=0.5, beta2=0.75))
    assert float((ref["p"] - rp2.detach()).abs().max()) <= 1e-12


# ------------------------------------------------------------------------------------------ momentum, nesterov, adam
def _chain(kind, c, mutate=None, nesterov=False):
    """three chained steps of the emulation, each held against the float64 statement applied to the state it started from -> worst ratios"""
    i = M.step_inputs(c)
    n = c["n"]
    state = dict(p=i["p"].clone(), ema=i["p"].clone() if c["ema"] else None)
    for k in (("buf",) if kind == "sgd" else ("m", "v")):
        state[k] = torch.zeros(n)
    worst = {}
    for step in (1, 2, 3):
        g = i["grads"][step - 1]
        gsq = (g * g).sum().reshape(1) if c["gnorm"] else None
        tail = (i["mask"], gsq, step, c["max_norm"], c["grad_scale"])
        if kind == "sgd":
            ref, bnd = M.sgd_step_bounds(state["p"], g, state["buf"], state["ema"], *tail, nesterov)
            e = M.sgd_step_emulate(state["p"], g, state["buf"], state["ema"], *tail, nesterov, mutate=mutate)
        else:
            ref, bnd = M.adam_step_bounds(state["p"], g, state["m"], state["v"], state["ema"], *tail)
            e = M.adam_step_emulate(state["p"], g, state["m"], state["v"], state["ema"], *tail, mutate=mutate)
        for k in ref:
            worst[k] = max(worst.get(k, 0.0), ratio(e[k], ref[k], bnd[k]))
        state.update(e)
    return worst


@pytest.mark.parametrize("nesterov", [False, True], ids=["momentum", "nesterov"])
@pytest.mark.parametrize("c", M.step_cases(), ids=_ids)
def test_sgd_emulation_within_bounds(c, nesterov):
    _hold(f"sgd nesterov={nesterov} {c}", _chain("sgd", c, nesterov=nesterov))


@pytest.mark.parametrize("c", M.step_cases(), ids=_ids)
def test_adam_emulation_within_bounds(c):
    _hold(f"adam {c}", _chain("adam", c))


@pytest.mark.parametrize("bug", M.SGD_MUTATIONS)
def test_sgd_planted_bugs(bug):
    hits = []
    for c in M.step_cases():
        if c["n"] > 100000:
            continue
        hits += [((c["n"], c["max_norm"], c["grad_scale"], c["mask"]), k, rt) for k, rt in _chain("sgd", c, mutate=bug, nesterov=True).items()]
    _caught(bug, hits)


@pytest.mark.parametrize("bug", M.ADAM_MUTATIONS)
def test_adam_planted_bugs(bug):
    hits = []
    for c in M.step_cases():
        if c["n"] > 100000:
            continue
        hits += [((c["n"], c["max_norm"], c["grad_scale"], c["mask"]), k, rt) for k, rt in _chain("adam", c, mutate=bug).items()]
    _caught(bug, hits)


# ------------------------------------------------------------------------------------------ the statements against torch.optim
# hyper-parameters that are exact in fp32 (the statements round them as the C ABI does), bias corrections included: 1 - 0.5^t and 1 - 0.75^t for t <= 3
EXACT_HP = dict(beta1=0.5, beta2=0.75, eps=2.0 ** -20, wd=0.0625, ema_decay=0.5, lr=2.0 ** -7, momentum=0.75)


def _two_groups(n, mask):
    """the flat vector as two torch parameter groups (decayed, exempt) -> (params, groups, scatter back)"""
    ex = mask.repeat_interleave(4).bool()
    return ex, (~ex).nonzero().flatten(), ex.nonzero().flatten()


@pytest.mark.parametrize("kind", ["momentum", "nesterov", "adam"])
@pytest.mark.parametrize("clipped", [False, True])
def test_statements_agree_with_torch(kind, clipped):
    n, hp = 64, EXACT_HP
    c = dict(n=n, max_norm=0.05, gnorm=True, grad_scale=1.0, mask=True, ema=False, p16=False)
    i = M.step_inputs(c)
    _, idx_d, idx_e = _two_groups(n, i["mask"])
    pd, pe = (i["p"].to(F64)[ix].clone().requires_grad_(True) for ix in (idx_d, idx_e))
    groups = [{"params": [pd], "weight_decay": hp["wd"]}, {"params": [pe], "weight_decay": 0.0}]
    if kind == "adam":
        opt = torch.optim.Adam(groups, lr=hp["lr"], betas=(hp["beta1"], hp["beta2"]), eps=hp["eps"])
    else:
        opt = torch.optim.SGD(groups, lr=hp["lr"], momentum=hp["momentum"], nesterov=kind == "nesterov")
    p = i["p"].to(F64)
    state = [torch.zeros(n, dtype=F64) for _ in range(2)]
    for step in (1, 2, 3):
        g = i["grads"][step - 1].to(F64)
        pd.grad, pe.grad = g[idx_d].clone(), g[idx_e].clone()
        gsq = None
        if clipped:
            gsq = (g * g).sum()
            torch.nn.utils.clip_grad_norm_([pd, pe], 0.0625)          # exact in fp32, as the statement takes it
        opt.step()
        tail = (None, i["mask"], gsq, step, 0.0625, 1.0)
        if kind == "adam":
            ref, _ = M.adam_step_bounds(p, g, state[0], state[1], *tail, hp=hp)
            state = [ref["m"], ref["v"]]
        else:
            ref, _ = M.sgd_step_bounds(p, g, state[0], *tail, kind == "nesterov", hp=hp)
            state = [ref["buf"], None]
        p = ref["p"]
        want = torch.empty(n, dtype=F64)
        want[idx_d], want[idx_e] = pd.detach(), pe.detach()
        rel = float(((p - want).abs() / want.abs().clamp_min(1e-30)).max())
        assert rel <= 1e-12, (kind, clipped, step, rel)


# ------------------------------------------------------------------------------------------ LAMB
def _lamb_chain(c, mutate=None):
    i = M.lamb_inputs(c)
    p, m, v = i["p"].clone(), i["m"].clone(), i["v"].clone()
    ema = i["p"].clone() if c["ema"] else None
    worst = {}
    for step in (1, 2, 3):
        g = i["grads"][step - 1]
        gsq = (g * g).sum().reshape(1)
        args = (i["layout"], gsq, step, c["max_norm"], c["grad_scale"], c["trust_clip"])
        ref, bnd = M.lamb_step_bounds(p, g, m, v, ema, *args)
        e = M.lamb_step_emulate(p, g, m, v, ema, *args, mutate=mutate)
        for k in ref:
            worst[k] = max(worst.get(k, 0.0), ratio(e[k], ref[k], bnd[k]))
        p, m, v, ema = e["p"], e["m"], e["v"], e.get("ema")
    return worst


def _lid(c):
    return f"{'lambc' if c['trust_clip'] else 'lamb'}-par{c['exempt_parity']}-mn{c['max_norm']}-gs{c['grad_scale']}"


@pytest.mark.parametrize("c", M.lamb_cases(), ids=_lid)
def test_lamb_emulation_within_bounds(c):
    _hold(f"lamb {c}", _lamb_chain(c))


@pytest.mark.parametrize("bug", M.LAMB_MUTATIONS)
def test_lamb_planted_bugs(bug):
    hits = []
    for c in M.lamb_cases():
        hits += [(_lid(c), k, rt) for k, rt in _lamb_chain(c, mutate=bug).items()]
    _caught(bug, hits)


@pytest.mark.parametrize("c", M.lamb_cases(), ids=_lid)
def test_lamb_statement_agrees_with_naive_loop(c):
    i = M.lamb_inputs(c)
    p, m, v = i["p"].to(F64), i["m"].to(F64), i["v"].to(F64)
    for step in (1, 2, 3):
        g = i["grads"][step - 1]
        gsq = (g.to(F64) ** 2).sum()
        args = (i["layout"], gsq, step, c["max_norm"], c["grad_scale"], c["trust_clip"])
        ref, _ = M.lamb_step_bounds(p, g, m, v, None, *args)
        nv = M.lamb_naive(p, g, m, v, *args)
        for k in ("p", "m", "v", "trust"):
            # relative to the terms that enter an element (m' = b1 m + (1 - b1) g'' cancels on some): the output's largest magnitude
            rel = float((ref[k] - nv[k]).abs().max() / nv[k].abs().max())
            assert rel <= 1e-12, (k, step, rel)
        p, m, v = ref["p"], ref["m"], ref["v"]


def test_lamb_properties():
    c = M.lamb_cases()[0]                                   # lamb (uncapped), even tensors exempt, no outer clip
    i = M.lamb_inputs(c)
    g = i["grads"][1]
    gsq = (g.to(F64) ** 2).sum()
    hp, lr = M.OPT_HP, T._f(M.OPT_HP["lr"])
    ref, _ = M.lamb_step_bounds(i["p"], g, i["m"], i["v"], None, i["layout"], gsq, 2, 0.0, 1.0, False)
    # the same gradients as LAMB hands them to its moments (norm clipped to 1), through Adam without decay
    g_seen = g.to(F64) / max(1.0, math.sqrt(float(gsq)))
    adam, _ = M.adam_step_bounds(i["p"], g_seen, i["m"], i["v"], None, None, None, 2, 1e9, 1.0, hp=dict(hp, wd=0.0))
    for si, (o, n, exempt) in enumerate(i["layout"]):
        sl = slice(o, o + n)
        p0, moved = i["p"].to(F64)[sl], (i["p"].to(F64) - ref["p"])[sl]
        if exempt:                                          # a no-decay tensor moves exactly as Adam without decay
            assert float(ref["trust"][si]) == 1.0
            assert float((ref["p"][sl] - adam["p"][sl]).abs().max()) <= 1e-12 * float(p0.abs().max())
        elif float(p0.norm()) > 0 and float(moved.norm()) > 0:      # ||lr trust u|| == lr ||p|| when uncapped
            assert abs(float(moved.norm()) - lr * float(p0.norm())) <= 1e-12 * lr * float(p0.norm()), si
        else:
            assert float(ref["trust"][si]) == 1.0, si
    assert float(ref["trust"][5]) == 1.0 and float(ref["trust"][6]) == 1.0          # p = 0 (g != 0); p = g = m = v = 0
    assert float((ref["p"][slice(*[i["layout"][6][0], i["layout"][6][0] + 8])]).abs().max()) == 0.0
    assert float(i["p"].to(F64)[slice(i["layout"][5][0], i["layout"][5][0] + 8)].abs().max()) == 0.0 \
        and float(ref["p"][slice(i["layout"][5][0], i["layout"][5][0] + 8)].abs().max()) > 0          # trust 1: the zero tensor still moves
    # lambc caps what lamb leaves above 1
    capped, _ = M.lamb_step_bounds(i["p"], g, i["m"], i["v"], None, i["layout"], gsq, 2, 0.0, 1.0, True)
    assert float(ref["trust"].max()) > 1.0 and float(capped["trust"].max()) == 1.0
    assert torch.equal(capped["trust"], ref["trust"].clamp_max(1.0))
    # the padding between tensors is nobody's: unchanged
    covered = torch.zeros(i["n"], dtype=torch.bool)
    for o, n, _ in i["layout"]:
        covered[o:o + n] = True
    assert bool((ref["p"][~covered] == M.GAP).all()) and bool((ref["m"][~covered] == M.GAP).all())
