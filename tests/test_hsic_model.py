"""tests/_hsic_model.py under test, on the CPU: on every case the fp32 emulation of a stage stays at |err| / bound <= 0.5 (below 1 on
_hsic_model.SHORT_PATHS, a few roundings of the output's own magnitude, where the bound is a correct implementation's worst case), every planted bug
reaches 1 on the output and case _hsic_model.MUTATIONS names for it, the float64 statements are the function shrink._hsic / _gauss_mix state (and
give the golden ranks), and devit_hsic_scores_workspace agrees with the case table.  A bound that its own emulation breaks is derived wrongly; a
bound that a planted bug passes is useless."""
import math
import os

import numpy as np
import pytest
import torch

import _hsic_model as M
from _hsic_model import F32, F64, ratio
from conftest import GOLDEN

HALF = 0.5
_STAGES = {}


def _hold(tag, res):
    print(tag, " ".join(f"{k} {v:.3f}" for k, v in res.items()))
    bad = {k: v for k, v in res.items() if not (v < 1.0 if k in M.SHORT_PATHS else v <= HALF)}
    assert not bad, f"{tag}: emulation |err| / bound {bad}"


def _stages(name):
    """the un-mutated pipeline of a score case, made once: inputs, ws, kmix1 (emulated, fp32) and the bounds of each stage"""
    if name not in _STAGES:
        c = M.case_by_name(name)
        i = M.score_inputs(c)
        ws = M.pack_emulate(i["X"], c["group"])
        k = M.kmix1_emulate(ws, c["B"])
        _STAGES[name] = dict(c=c, i=i, ws=ws, k=k, pack=M.pack_bounds(i["X"], c["group"]), kmix1=M.kmix1_bounds(ws[:, :, :c["B"]]))
    return _STAGES[name]


NAMES = [c["name"] for c in M.score_cases()]


@pytest.mark.parametrize("name", NAMES)
def test_score_emulations_within_bounds(name):
    s = _stages(name)
    c, i, ws, k = s["c"], s["i"], s["ws"], s["k"]
    B, group = c["B"], c["group"]
    res = {}
    ref, bnd = s["pack"]
    if group == 1:
        assert torch.equal(ws[:, :, :B], i["X"].to(F32).permute(2, 1, 0)) and float(bnd.max()) == 0.0
    else:
        res["ws"] = ratio(ws[:, :, :B], ref, bnd)
    assert bool((ws[:, :, B:] == 0).all())
    kref, kbnd = s["kmix1"]
    res["kmix1"] = ratio(k, kref, kbnd)
    assert bool((torch.diagonal(k, dim1=1, dim2=2) == 0).all())          # symmetry to the bit is the kernel's property (one k, two stores)
    res["rel"] = ratio(M.rel_emulate(k, i["W"]), *M.rel_bounds(k, i["W"]))
    if group == 1:
        res["act"] = ratio(M.act_emulate(ws), *M.act_bounds(ws))
    else:
        res["red"] = ratio(M.red_emulate(k), *M.red_bounds(k))
    _hold(name, res)
    # a masked unit (regime 4) is exactly zero in every output; so is the kernel of coinciding samples (regime 5 at one token)
    for u in range(4, c["units"], 6):
        assert not bool(k[u].any()) and float(M.rel_emulate(k, i["W"])[u]) == 0.0 and float(kbnd[u].max()) == 0.0
        assert group != 1 or float(M.act_emulate(ws)[u]) == 0.0
    if c["N"] == 1 and c["units"] > 5:
        assert not bool(k[5].any()) and float(kbnd[5].max()) == 0.0


def test_every_regime_and_branch_is_reached():
    """the case table does put elements on both branches of expm1_neg for every Gaussian, at the underflow of the narrowest one and at d2 == 0"""
    seen = set()
    for name in ("B64_N3_u6_g1_f32_contig", "B5_N67_u6_g1_f32_offset", "B256_N3_u6_g1_f32_contig"):
        s = _stages(name)
        dd = M.d2(s["ws"][:, :, :s["c"]["B"]])
        for j, c in enumerate(M.COEF):
            seen |= {("taylor", j)} if bool(((c * dd < 0.25) & (dd > 0)).any()) else set()
            seen |= {("exp2", j)} if bool((c * dd > 0.25).any()) else set()
        seen |= {"underflow"} if bool((0.5 * dd > 104).any()) else set()
        seen |= {"zero"} if bool((dd == 0).any()) else set()
    assert seen == {("taylor", j) for j in range(5)} | {("exp2", j) for j in range(5)} | {"underflow", "zero"}, seen


def test_head_pairs_emulation_on_a_synthetic_kernel():
    k = M.synthetic_kmix1()
    assert torch.equal(k, k.transpose(1, 2)) and float(k.min()) >= -1.0 and float(k[k != 0].max()) <= -9e-8
    _hold("synthetic kmix1", {"red": ratio(M.red_emulate(k), *M.red_bounds(k))})


TNAMES = [c["name"] for c in M.target_cases()]


@pytest.mark.parametrize("name", TNAMES)
def test_target_emulation_within_bounds(name):
    c = M.case_by_name(name)
    y = M.target_inputs(c)
    ref, bnd = M.target_bounds(y, c["softmax"])
    _hold(name, {"W": ratio(M.target_emulate(y, c["softmax"]), ref, bnd)})
    if c["C"] == 1 and c["softmax"]:
        assert not bool(M.target_emulate(y, 1).any()) and float(ref.abs().max()) == 0.0          # one class: p = 1, z = 0


def _mutated(bug):
    """the ratio (or inf for a torch.equal / exact-zero mismatch) of the planted bug on the output and case MUTATIONS names"""
    name, out = M.MUTATIONS[bug]
    if bug in M.TARGET_MUTATIONS:
        c = M.case_by_name(name)
        y = M.target_inputs(c)
        return ratio(M.target_emulate(y, c["softmax"], mutate=bug), *M.target_bounds(y, c["softmax"]))
    s = _stages(name)
    c, i = s["c"], s["i"]
    if bug in M.PACK_MUTATIONS:
        ws = M.pack_emulate(i["X"], c["group"], mutate=bug)
        return ratio(ws[:, :, :c["B"]], *s["pack"]) if out == "ws" else ratio(M.act_emulate(ws), *M.act_bounds(s["ws"]))
    if bug in M.HEAD_MUTATIONS:
        return ratio(M.red_emulate(s["k"], mutate=bug), *M.red_bounds(s["k"]))
    if bug == "offdiag_tiles_once":
        return ratio(M.rel_emulate(s["k"], i["W"], mutate=bug), *M.rel_bounds(s["k"], i["W"]))
    return ratio(M.kmix1_emulate(s["ws"], c["B"], mutate=bug), *s["kmix1"])


@pytest.mark.parametrize("bug", sorted(M.MUTATIONS))
def test_planted_bug_is_caught(bug):
    assert set(M.MUTATIONS) == set(M.PAIR_MUTATIONS + M.PACK_MUTATIONS + M.TARGET_MUTATIONS + M.HEAD_MUTATIONS)
    rt = _mutated(bug)
    print(f"planted bug {bug}: {M.MUTATIONS[bug][0]} / {M.MUTATIONS[bug][1]}: ratio {rt:.3g}")
    assert rt >= 1.0, f"planted bug {bug} passes the bound of {M.MUTATIONS[bug]}: ratio {rt:.3g}"


def test_pad_not_zeroed_is_seen_by_act_alone():
    """the pair loop masks a < B and b < B, so kmix1 and rel never read the pad; act sums whole tiles"""
    s = _stages(M.MUTATIONS["pad_not_zeroed"][0])
    ws = M.pack_emulate(s["i"]["X"], 1, mutate="pad_not_zeroed")
    assert torch.equal(M.kmix1_emulate(ws, s["c"]["B"]), s["k"]) and not bool(torch.isfinite(M.act_emulate(ws)).any())


def test_statements_are_the_repository_restatement():
    """on inputs without constant non-zero columns (regimes 0 .. 4) the stage statements composed are shrink._hsic / _gauss_mix, in float64, to the
    1e-6 of the largest value that test_scores_of_a_real_forward applies to the same comparison"""
    from devit_amd import shrink
    for name in ("B5_N34_u6_g1_f32_contig", "B63_N3_u6_g1_f16_contig", "B129_N34_u6_g8_f32_batch_pad"):
        c = M.case_by_name(name)
        i = M.score_inputs(c)
        x = M.features(i["X"], c["group"])
        keep = [u for u in range(c["units"]) if u % 6 != 5]
        x = x[keep]
        prob = torch.softmax(i["logits"].to(F64), -1)
        xs = x.permute(0, 2, 1)                                              # [units][B][N]: shrink's layout
        k = M.kmix1(x)
        gm = shrink._gauss_mix(xs)
        assert float((k + 1 - gm).abs().max()) <= 1e-6 * float(gm.abs().max())
        ref = shrink._hsic(xs, prob, 'linear', True)
        got = M.rel(k, M.target(prob, False))
        assert float((got - ref).abs().max()) <= 1e-6 * float(ref.abs().max()), name
        assert float((M.target(i["logits"], True) - M.target(prob, False)).abs().max()) <= 1e-12
        if c["group"] > 1:
            H = len(keep)
            rr = torch.stack([sum(shrink._hsic(xs[a], xs[b], 'rbf', False) for b in range(H) if b != a) / (H - 1) for a in range(H)])
            assert float((M.red(k) - rr).abs().max()) <= 1e-6 * float(rr.abs().max()), name


def test_golden_ranks_from_the_statements():
    g = dict(np.load(os.path.join(GOLDEN, "imp_rank.npz")))
    prob = torch.softmax(torch.from_numpy(g["logits"]).to(F64), -1)
    W = M.target(prob, False)
    mm = lambda v: (v - v.min()) / (v.max() - v.min())
    for i in range(2):
        x = M.features(torch.from_numpy(g[f"n{i}"]), 1)
        ns = 0.1 * mm(M.rel(M.kmix1(x), W)) + 0.9 * mm(M.act(x))
        assert np.array_equal(np.argsort(ns.numpy()), g["neuron_rank"][i])
        h = torch.from_numpy(g[f"h{i}"])
        k = M.kmix1(M.features(h.reshape(h.shape[0], h.shape[1], -1), h.shape[3]))
        hs = M.rel(k, W) - 0.1 * M.red(k)
        assert np.array_equal(np.argsort(hs.numpy()), g["head_rank"][i])


def test_workspace_query_against_the_case_table():
    from devit_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = _lib.load()
    for c in M.score_cases():
        assert lib.devit_hsic_scores_workspace(c["B"], c["N"], c["units"]) == M.workspace_bytes(c["B"], c["N"], c["units"]), c["name"]
        off, sb, sn, total = M.strides_of(c)
        ch = c["units"] * c["group"]
        assert sn >= ch and sb >= (c["N"] - 1) * sn + ch and total > off + (c["B"] - 1) * sb + (c["N"] - 1) * sn + ch - 1
    assert lib.devit_hsic_scores_workspace(M.MAX_B + 1, 3, 6) == 0 and math.isclose(M.U, 2.0 ** -24)
