"""tests/_tail_model.py under test, on the CPU: on every case the fp32 emulation of a kernel stays at |err| / bound <= 0.5 under every bound (below 1
on the 16-bit stores and the few short paths _tail_model.SHORT_PATHS lists, where a correct implementation attains the bound's worst case), every
planted bug reaches 1 on a named output of a named case (or breaks torch.equal where the case is exact), and the float64 statements agree with
torch's own ops to 1e-12.  A bound that its own emulation breaks is derived wrongly; a bound that a planted bug passes is useless."""
import math

import pytest
import torch

import _tail_model as T
from _tail_model import BF16, F16, F32, F64, ratio

HALF = 0.5


def _hold(tag, res):
    """fp32 outputs at <= 0.5; below 1 for outputs stored in a 16-bit type (names ending in 16: a correct rounding alone comes close to its term)
    and for _tail_model.SHORT_PATHS (a few roundings of the output's own magnitude: the bound is a correct implementation's worst case)"""
    print(tag, " ".join(f"{k} {v:.3f}" for k, v in res.items()))
    bad = {k: v for k, v in res.items() if not (v < 1.0 if (k.endswith("16") or k in T.SHORT_PATHS) else v <= HALF)}
    assert not bad, f"{tag}: emulation |err| / bound {bad}"


def _caught(bug, hits):
    """hits: list of (case, output, ratio)"""
    hits = [h for h in hits if h[2] >= 1.0]
    assert hits, f"planted bug {bug}: not caught on any output of any case"
    case, out, rt = max(hits, key=lambda h: h[2])
    print(f"planted bug {bug}: caught on {len(hits)} (case, output) pairs; worst {case} / {out}: ratio {rt:.3g}")


# ------------------------------------------------------------------------------------------ LayerNorm
def _ln_fwd_stats(D, rows):
    i = T.ln_inputs(D, rows)
    e = T.ln_fwd_emulate(i["x"], i["gamma"], i["beta"])
    return i, e


@pytest.mark.parametrize("D,rows", T.ln_cases())
def test_ln_forward_emulation_within_bounds(D, rows):
    i, e = _ln_fwd_stats(D, rows)
    ref, bnd = T.ln_fwd_bounds(i["x"], i["gamma"], i["beta"])
    res = {k: ratio(e[k], ref[k], bnd[k]) for k in ("y", "mean", "rstd")}
    res["y_bf16"] = ratio(e["y"].to(BF16), ref["y"], T.stored16(bnd["y"], ref["y"]))
    res["y_f16"] = ratio(e["y"].to(F16), ref["y"], T.stored16(bnd["y"], ref["y"], f16=True))
    _hold(f"ln_fwd D{D} rows{rows}", res)
    const = i["regime"] == 3
    if bool(const.any()):          # a constant row: rstd = eps^-1/2 and y = beta, both within their bounds
        assert torch.allclose(ref["rstd"][const], torch.full_like(ref["rstd"][const], T._f(T.LN_EPS) ** -0.5), rtol=1e-12)
        assert torch.allclose(ref["y"][const], i["beta"].to(F64).expand(int(const.sum()), D), atol=1e-9)


def test_ln_forward_planted_bug():
    hits = []
    for D, rows in T.ln_cases():
        i = T.ln_inputs(D, rows)
        ref, bnd = T.ln_fwd_bounds(i["x"], i["gamma"], i["beta"])
        e = T.ln_fwd_emulate(i["x"], i["gamma"], i["beta"], mutate="one_pass_variance")
        hits += [((D, rows), k, ratio(e[k], ref[k], bnd[k])) for k in ("y", "rstd")]
    _caught("one_pass_variance", hits)
    # where it shows: mean 1000, std 0.01 (the issue's figure: far outside the elementwise bound)
    i = T.ln_inputs(384, 250)
    ref, bnd = T.ln_fwd_bounds(i["x"], i["gamma"], i["beta"])
    e = T.ln_fwd_emulate(i["x"], i["gamma"], i["beta"], mutate="one_pass_variance")
    rows1 = i["regime"] == 1
    assert ratio(e["y"][rows1], ref["y"][rows1], bnd["y"][rows1]) > 10


@pytest.mark.parametrize("D,rows", T.ln_cases())
def test_ln_backward_emulation_within_bounds(D, rows):
    i, f = _ln_fwd_stats(D, rows)
    for dres, acc in ((i["dres"], True), (None, False)):
        g0, b0 = (i["dgamma0"], i["dbeta0"]) if acc else (None, None)
        ref, bnd = T.ln_bwd_bounds(i["x"], f["mean"], f["rstd"], i["gamma"], i["dy"], dres, g0, b0)
        e = T.ln_bwd_emulate(i["x"], f["mean"], f["rstd"], i["gamma"], i["dy"], dres, g0, b0)
        res = {k: ratio(e[k], ref[k], bnd[k]) for k in ("dx", "dgamma", "dbeta")}
        dxb = e["dx"].to(BF16)
        cs, ecs = T.ln_colsum_bounds(dxb, i["colsum0"] if acc else None)
        got = dxb.to(F32).sum(0) + (i["colsum0"] if acc else 0)
        res["colsum"] = ratio(got, cs, ecs)
        _hold(f"ln_bwd D{D} rows{rows} dres{dres is not None}", res)


@pytest.mark.parametrize("bug", T.LN_BWD_MUTATIONS)
def test_ln_backward_planted_bugs(bug):
    hits = []
    for D, rows in T.ln_cases():
        if rows > 250:
            continue
        i, f = _ln_fwd_stats(D, rows)
        ref, bnd = T.ln_bwd_bounds(i["x"], f["mean"], f["rstd"], i["gamma"], i["dy"], i["dres"])
        e = T.ln_bwd_emulate(i["x"], f["mean"], f["rstd"], i["gamma"], i["dy"], i["dres"], mutate=bug)
        hits.append(((D, rows), "dx", ratio(e["dx"], ref["dx"], bnd["dx"])))
    _caught(bug, hits)


def test_ln_statements_agree_with_torch():
    i = T.ln_inputs(192, 9)
    i["x"] = T.randn(T.gen("ln_torch"), 9, 192) * 2 + 0.5          # torch's own float64 kernel is the imprecise side at mean 1e4
    x = i["x"].to(F64).requires_grad_(True)
    gm, bt = i["gamma"].to(F64).requires_grad_(True), i["beta"].to(F64).requires_grad_(True)
    y = torch.nn.functional.layer_norm(x, (192,), gm, bt, T._f(T.LN_EPS))
    ref = T.ln_fwd_ref(i["x"], i["gamma"], i["beta"])
    assert float((y.detach() - ref["y"]).abs().max()) <= 1e-12 * float(y.detach().abs().max())
    y.backward(i["dy"].to(F64))
    b = T.ln_bwd_ref(i["x"].to(F64), ref["mean"], ref["rstd"], i["gamma"], i["dy"], i["dres"])
    for got, want in ((b["dx"] - i["dres"].to(F64), x.grad), (b["dgamma"], gm.grad), (b["dbeta"], bt.grad)):
        assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))


# ------------------------------------------------------------------------------------------ sgemm_small
@pytest.mark.parametrize("c", T.sgemm_cases(), ids=lambda c: f"K{c['K']}-{c['M']}x{c['N']}-{c['form']}-{'int' if c['ints'] else 'rnd'}")
def test_sgemm_small_emulation(c):
    i = T.sgemm_inputs(c)
    ref, bnd = T.sgemm_bounds(i["A"], i["B"], i["bias"], i["C0"], c["alpha"], c["accumulate"])
    e = T.sgemm_emulate(i["A"], i["B"], i["bias"], i["C0"], c["alpha"], c["accumulate"])
    if c["ints"]:
        assert torch.equal(e.to(F64), ref)
    else:
        _hold(f"sgemm {c}", dict(C=ratio(e, ref, bnd)))


def test_sgemm_small_planted_bug():
    hits, exact_hits = [], []
    for c in T.sgemm_cases():
        i = T.sgemm_inputs(c)
        ref, bnd = T.sgemm_bounds(i["A"], i["B"], i["bias"], i["C0"], c["alpha"], c["accumulate"])
        e = T.sgemm_emulate(i["A"], i["B"], i["bias"], i["C0"], c["alpha"], c["accumulate"], mutate="tail_k_dropped")
        if c["ints"]:
            if not torch.equal(e.to(F64), ref):
                exact_hits.append(c["K"])
        else:
            hits.append(((c["K"], c["M"], c["N"]), "C", ratio(e, ref, bnd)))
    _caught("tail_k_dropped", hits)
    print("planted bug tail_k_dropped: exact-integer mismatch at K =", exact_hits)
    assert 64 not in exact_hits and len(set(exact_hits)) >= 5
    assert all(h[2] < 1 for h in hits if h[0][0] == 64), "K = 64 has no tail: the existing K = 384 test's blind spot"


# ------------------------------------------------------------------------------------------ colsum
def test_colsum_statement_and_planted_bug():
    broke = []
    for M, N, grp, skip, acc in T.colsum_cases():
        i = T.colsum_inputs(M, N, grp, skip)
        ref = T.colsum_ref(i["y"], M, N, grp, skip, i["out0"] if acc else None)
        assert bool(torch.isfinite(ref).all()) and torch.equal(ref, ref.round())
        mut = T.colsum_ref(i["y"], M, N, grp, skip, i["out0"] if acc else None, mutate="skip_not_applied")
        if grp:
            assert not torch.equal(mut, ref)
            broke.append((M, N, grp, skip))
        else:
            assert torch.equal(mut, ref)
    print("planted bug skip_not_applied: torch.equal mismatch on", broke)
    assert broke


# ------------------------------------------------------------------------------------------ logit loss
_CLS_IDS = [f"B{B}-C{C}-k{k}-a{a}-t{t}-{v}" for B, C, k, a, t, v in T.cls_cases()]


@pytest.mark.parametrize("B,C,kind,alpha,tau,variant", T.cls_cases(), ids=_CLS_IDS)
def test_cls_loss_emulation_within_bounds(B, C, kind, alpha, tau, variant):
    i = T.cls_inputs(B, C, variant)
    ref, bnd = T.cls_bounds(i["lo"], i["lk"], i["lt"], i["y"], kind, alpha, tau)
    e = T.cls_emulate(i["lo"], i["lk"], i["lt"], i["y"], kind, alpha, tau)
    _hold(f"cls B{B} C{C} kind{kind} {variant}", {k: ratio(e[k], ref[k], bnd[k]) for k in ("loss3", "dlo", "dlk")})
    if kind == T.KIND_NONE:
        assert not bool(ref["dlk"].any()) and not bool(e["dlk"].any())


@pytest.mark.parametrize("bug", T.CLS_MUTATIONS)
def test_cls_loss_planted_bugs(bug):
    hits = []
    for B, C, kind, alpha, tau, variant in T.cls_cases():
        i = T.cls_inputs(B, C, variant)
        ref, bnd = T.cls_bounds(i["lo"], i["lk"], i["lt"], i["y"], kind, alpha, tau)
        e = T.cls_emulate(i["lo"], i["lk"], i["lt"], i["y"], kind, alpha, tau, mutate=bug)
        hits += [((B, C, kind, variant), k, ratio(e[k], ref[k], bnd[k])) for k in ("loss3", "dlo", "dlk")]
    _caught(bug, hits)
    want = "tie" if bug == "tie_highest_index" else "soft07"
    assert all(want in h[0][3] for h in hits if h[2] >= 1), "the bug shows only where the inputs reach it"
    if bug == "tie_highest_index":
        assert {h[0][3] for h in hits if h[2] >= 1} == {"tie_two_lanes", "tie_one_lane"}


def test_cls_statement_agrees_with_torch():
    B, C = 17, 65
    i = T.cls_inputs(B, C, "soft07")
    lo, lk, lt, y = (i[k].to(F64) for k in ("lo", "lk", "lt", "y"))
    for kind, tau in ((T.KIND_HARD, 1.0), (T.KIND_SOFT, 3.0), (T.KIND_NONE, 1.0)):
        a, k = lo.clone().requires_grad_(True), lk.clone().requires_grad_(True)
        base = torch.sum(-y * torch.log_softmax(a, -1), -1).mean()
        if kind == T.KIND_HARD:
            dist = torch.nn.functional.cross_entropy(k, lt.argmax(1))
        elif kind == T.KIND_SOFT:
            dist = torch.nn.functional.kl_div(torch.log_softmax(k / tau, 1), torch.log_softmax(lt / tau, 1), reduction="sum",
                                              log_target=True) * tau * tau / k.numel()
        else:
            dist = 0.0 * k.sum()
        total = base if kind == T.KIND_NONE else 0.75 * base + 0.25 * dist
        total.backward()
        total, base = total.detach(), base.detach()
        r = T.cls_ref(lo, lk, lt, y, kind, 0.25, tau)
        assert abs(float(r["loss3"][0] - total)) <= 1e-12 * max(1, abs(float(total)))
        assert abs(float(r["loss3"][1] - base)) <= 1e-12 * abs(float(base))
        assert float((r["dlo"] - a.grad).abs().max()) <= 1e-12
        assert float((r["dlk"] - (k.grad if k.grad is not None else 0)).abs().max()) <= 1e-12


# ------------------------------------------------------------------------------------------ token MSE
@pytest.mark.parametrize("n", T.MSE_NS)
def test_mse(n):
    i = T.mse_inputs(n)
    for l0 in (None, i["loss0"]):
        ref, bnd = T.mse_bounds(i["a"], i["b"], l0)
        e = T.mse_emulate(i["a"], i["b"], l0)
        _hold(f"mse n{n} acc{l0 is not None}", {k: ratio(e[k], ref[k], bnd[k]) for k in ("loss", "da")})
    a = i["a"].to(F64).requires_grad_(True)
    l = torch.nn.functional.mse_loss(a, i["b"].to(F64))
    l.backward()
    l = l.detach()
    ref, _ = T.mse_bounds(i["a"], i["b"])
    assert abs(float(ref["loss"] - l)) <= 1e-12 * float(l) and float((ref["da"] - a.grad).abs().max()) <= 1e-12


# ------------------------------------------------------------------------------------------ relation loss
@pytest.mark.parametrize("B,N,hd_t,hd_s,scale", T.rel_cases())
def test_relation_emulation_within_bounds(B, N, hd_t, hd_s, scale):
    i = T.rel_inputs(B, N, hd_t, hd_s, scale)
    ref, bnd = T.rel_stats_bounds(i["gram_t"], i["gram_s"], hd_t, hd_s)
    e = T.rel_stats_emulate(i["gram_t"], i["gram_s"], hd_t, hd_s)
    res = {k: ratio(e[k], ref[k], bnd[k]) for k in ("lse_t", "lse_s", "row_kl", "loss")}
    for up, b16 in ((None, True), (0.37, False)):
        S, eS = T.rel_grad_bounds(i["gram_t"], i["gram_s"], e["lse_t"], e["lse_s"], up, hd_t, hd_s, b16)
        got = T.rel_grad_emulate(i["gram_t"], i["gram_s"], e["lse_t"], e["lse_s"], up, hd_t, hd_s, b16)
        res["S_bf16" if b16 else "S_f32"] = ratio(got, S, eS)
    _hold(f"relation B{B} N{N} hd({hd_t},{hd_s}) {scale}", res)


@pytest.mark.parametrize("std", [0.25, 1.0])
def test_relation_loss_from_features(std):
    """the bound test_gpu_kernels.test_relation_loss holds the loss value to: fp32 Grams (any summation order) and the fp32 emulation stay inside"""
    g = T.gen("rel_feat", std)
    B, N = 3, 198
    fs, ft = (T.randn(g, B, N, 128) * std).to(BF16), (T.randn(g, B, N, 256) * std).to(BF16)
    want, bound = T.rel_feature_loss_bounds(fs.to(F64).cpu(), ft.to(F64), 64, 64)
    gt, gs = ft.to(F32) @ ft.to(F32).transpose(1, 2), fs.to(F32) @ fs.to(F32).transpose(1, 2)
    e = T.rel_stats_emulate(gt, gs, 64, 64)
    _hold(f"relation loss from features std{std}", dict(loss=ratio(e["loss"], want, bound)))
    print(f"loss {float(want):.6e} bound {float(bound):.3e} ({float(bound / want):.2e} relative)")
    assert float(bound) < float(want), "the bound is not vacuous: it resolves the loss value"


def test_relation_statement_agrees_with_torch():
    i = T.rel_inputs(3, 198, 64, 32, "unit")
    ref, _ = T.rel_stats_bounds(i["gram_t"], i["gram_s"], 64, 32)
    t = torch.log_softmax(i["gram_t"].to(F64) / 8, -1)
    s = torch.log_softmax(i["gram_s"].to(F64) / math.sqrt(32), -1)
    want = torch.nn.functional.kl_div(s, t, reduction="sum", log_target=True) / 3
    assert abs(float(ref["loss"] - want)) <= 1e-12 * max(1.0, abs(float(want)))


# ------------------------------------------------------------------------------------------ exact-fp32 companions
@pytest.mark.parametrize("rows", T.SOFTMAX_ROWS)
@pytest.mark.parametrize("ncols", T.SOFTMAX_COLS)
def test_softmax_emulation_within_bounds(rows, ncols):
    i = T.softmax_inputs(rows, ncols)
    ref, bnd = T.softmax_bounds(i["S"], i["scale"])
    e = T.softmax_emulate(i["S"], i["scale"])
    res = {k: ratio(e[k], ref[k], bnd[k]) for k in ("P", "lse")}
    dS, edS = T.softmax_bwd_bounds(e["P"], i["dP"], i["scale"])
    P32, dP32 = e["P"], i["dP"]
    got = torch.tensor(i["scale"], dtype=F32) * P32 * (dP32 - (P32 * dP32).sum(1, keepdim=True))
    res["dS"] = ratio(got, dS, edS)
    _hold(f"softmax {rows}x{ncols}", res)
    want = torch.softmax(i["S"].to(F64) * T._f(i["scale"]), 1)
    assert float((ref["P"] - want).abs().max()) <= 1e-12


def test_gelu_statements():
    v = torch.linspace(-6, 6, 241, dtype=F64).requires_grad_(True)
    y = torch.nn.functional.gelu(v)
    y.sum().backward()
    assert float((T.gelu64(v.detach()) - y.detach()).abs().max()) <= 1e-12
    assert float((T.dgelu64(v.detach()) - v.grad).abs().max()) <= 1e-12
    v32 = v.detach().to(F32)
    got = 0.5 * v32 * (1 + torch.erf(v32 * torch.tensor(0.70710678118654752, dtype=F32)))
    assert ratio(got, T.gelu64(v32.to(F64)), T.gelu_bound(v32.to(F64), torch.zeros_like(v32, dtype=F64))) <= HALF
