"""tests/_block_model.py under test, without a GPU: the fp32 emulation of one encoder block passes the stage audit, every planted wiring bug is seen
on the stage it is named for (or by the untouched-bytes statement it breaks), the buffer extents include/devit_hip.h words are what
devit_block_acts_sizes / devit_block_bwd_sizes report, and the entry points' refusals -- argument checks in front of the first launch, so they
need no device -- return their DEVIT_ERR_* with the cause in the message.  tests/test_gpu_block.py runs the same audit on the sequence itself.
The lean last block (devit_tail_fwd / devit_tail_bwd) likewise: tail_emulate under tail_audit on the six cases of the tail table, and every entry
of TAIL_MUTATIONS seen where it is named; tests/test_gpu_tail_call.py runs that audit on the two calls."""
import functools

import pytest
import torch

import _block_model as K

BWD_CASES = [c for c in K.CASES if c["flags"] & K.SAVE]
# stages that are 16-bit stores (held below 1 like every 16-bit store of the sibling models: a correct round-to-nearest store comes arbitrarily close
# to its own term of the bound); every fp32 stage stays at <= 0.5
STORES16 = {"ln1", "qkv", "attn_o", "att", "ln2", "h", "h_pre", "dh_pre", "dln2", "g1", "dattn", "dqkv", "dln1", "g_prev"}


@functools.lru_cache(maxsize=None)
def clean(name):
    """(inputs, unmutated emulation, its audit) of a case: computed once, shared, left unchanged"""
    c = K.case_named(name)
    inp = K.inputs(c)
    bufs = K.emulate(c, inp)
    return inp, bufs, K.audit(c, inp, bufs, K.default_routes(c) if c["flags"] & K.SAVE else None)


@pytest.mark.parametrize("c", K.CASES, ids=[c["name"] for c in K.CASES])
def test_emulation_passes_the_stage_audit(c):
    _, _, (rt, problems) = clean(c["name"])
    print(" ".join(f"{k} {v:.3f}" for k, v in rt.items()))
    assert not problems, problems
    for name, r in rt.items():
        assert r < 1.0 if name in STORES16 else r <= 0.5, (c["name"], name, r)
    if c["flags"] & K.SAVE:       # the whole list of the sequence: nothing the block leaves in memory is unaudited
        want = {"ln1", "mean1", "rstd1", "qkv", "attn_o", "lse", "x1", "ln2", "mean2", "rstd2", "h", "h_pre", "x2", "fc2_b", "fc2_w", "dh_pre", "dln2",
                "fc1_w", "fc1_b", "dx1", "g1", "n2w", "n2b", "proj_b", "dattn", "proj_w", "dqkv", "dln1", "qkv_w", "qkv_b", "dx_in", "n1w", "n1b", "g_prev",
                "prev_fc2_b"} | ({"att"} if c["flags"] & K.ATT else set())
        assert set(rt) == want, set(rt) ^ want


@pytest.mark.parametrize("mutate", sorted(set(K.MUTATIONS) - set(K.DROP_MUTATIONS)))
@pytest.mark.parametrize("c", BWD_CASES, ids=[c["name"] for c in BWD_CASES])
def test_planted_wiring_bug_is_seen(c, mutate):
    inp, _, _ = clean(c["name"])
    rt, problems = K.audit(c, inp, K.emulate(c, inp, mutate=mutate), K.default_routes(c))
    where = K.MUTATIONS[mutate]
    if where in ("pad_rows", "inputs"):
        assert any(p.startswith(where + "/") for p in problems), (mutate, problems)
        if where == "pad_rows":
            assert {"pad_rows/h", "pad_rows/g1"} <= set(problems)
    else:
        assert rt[where] >= 1.0, (c["name"], mutate, where, rt[where])


# ---- the dropped sequence (devit_encoder_fwd_drop / devit_block_bwd_drop)
DROP_VARIANTS = K.drop_variants()
# one run per (case, rates): the environment switches choose kernels, not wires, and the CPU emulation has no kernels to choose
DROP_RUNS = list({(v[1]["name"], v[3]["p"], v[3]["p_attn"]): v for v in DROP_VARIANTS}.values())
ALL_STAGES = {"ln1", "mean1", "rstd1", "qkv", "attn_o", "lse", "x1", "ln2", "mean2", "rstd2", "h", "h_pre", "x2", "fc2_b", "fc2_w", "dh_pre", "dln2",
              "fc1_w", "fc1_b", "dx1", "g1", "n2w", "n2b", "proj_b", "dattn", "proj_w", "dqkv", "dln1", "qkv_w", "qkv_b", "dx_in", "n1w", "n1b", "g_prev",
              "prev_fc2_b"}


@functools.lru_cache(maxsize=None)
def clean_drop(name, p, p_attn):
    c = K.case_named(name)
    drop = K.drop_of(c["block"], p, p_attn)
    inp = K.inputs(c)
    route = K.default_routes(c, drop=drop)
    bufs = K.emulate(c, inp, route=route, drop=drop)
    return c, drop, inp, route, bufs, K.audit(c, inp, bufs, route, drop=drop)


def applies(need, drop):
    return {"p": drop["p"] > 0, "p_attn": drop["p_attn"] > 0, "p != p_attn": drop["p"] > 0 and drop["p"] != drop["p_attn"]}[need]


@pytest.mark.parametrize("tag,c,env,drop", DROP_RUNS, ids=[v[0] for v in DROP_RUNS])
def test_dropped_emulation_passes_the_stage_audit(tag, c, env, drop):
    _, _, _, route, bufs, (rt, problems) = clean_drop(c["name"], drop["p"], drop["p_attn"])
    print(" ".join(f"{k} {v:.3f}" for k, v in rt.items()))
    assert not problems, problems
    # x2 under p > 0 is as tight as a 16-bit store: devit_dropout_residual's bound counts exactly its two roundings (y * s, the fma), and the
    # emulation makes the same two
    for name, r in rt.items():
        assert r < 1.0 if name in STORES16 or (name == "x2" and drop["p"] > 0) else r <= 0.5, (tag, name, r)
    assert set(rt) == ALL_STAGES | ({"tmp"} if drop["p"] > 0 else set()), set(rt) ^ ALL_STAGES
    assert (route["fc2_bias"] == "masked") == (drop["p"] > 0)
    if drop["p"] > 0:
        M = K.dims(c)["M"]
        for name, site, cols in (("h", K.SITE_HIDDEN, c["hidden"]), ("dh_pre", K.SITE_HIDDEN, c["hidden"]), ("g1", K.SITE_PROJ, c["D"])):
            keep = K.site_keep(c, drop, site, cols)
            frac = 1 - float(keep.float().mean())
            assert abs(frac - drop["p"]) < 0.01 and bool((bufs[name][:M][~keep] == 0).all()), (name, frac)


DROP_PLANTED = [(v, m) for v in DROP_RUNS for m in sorted(K.DROP_MUTATIONS) if applies(K.DROP_MUTATIONS[m][1], v[3])]


@pytest.mark.parametrize("v,mutate", DROP_PLANTED, ids=[f"{v[0]}-{m}" for v, m in DROP_PLANTED])
def test_planted_dropout_wiring_bug_is_seen(v, mutate):
    _, c, _, drop = v
    _, _, inp, route, _, _ = clean_drop(c["name"], drop["p"], drop["p_attn"])
    rt, problems = K.audit(c, inp, K.emulate(c, inp, mutate=mutate, route=route, drop=drop), route, drop=drop)
    where = K.MUTATIONS[mutate]
    if where.startswith("inputs/"):
        assert where in problems, (mutate, problems)
    else:
        assert rt[where] >= 1.0, (c["name"], mutate, where, rt[where])


def test_every_dropout_mutation_meets_a_case():
    assert {m for _, m in DROP_PLANTED} == set(K.DROP_MUTATIONS)
    assert {v[3]["block"] for v in DROP_VARIANTS} == {0, 5, 11}, "block indices other than 0, so that a dropped `block` argument shows"
    assert all(c["flags"] & K.ATT == 0 and K.dims(c)["M"] % 256 for c in K.DROP_CASES)


def test_inputs_make_a_swapped_wire_visible():
    """what the issue asks of the inputs, stated once"""
    for c in BWD_CASES:
        w, inp = K.block_weights(c), clean(c["name"])[0]
        assert not torch.equal(w["dp1"], w["dp2"])
        for v in (w["dp1"], w["dp2"]):
            assert bool((v == 0).any()) and bool((v > 1).any())
        assert bool((w["head_gate"] == 0).any()) and bool((w["head_gate"] > 1).any())
        assert bool((w["neuron_gate"] == 0).any()) and bool((w["neuron_gate"] < 0).any()) and bool((w["neuron_gate"] > 1).any())
        for b in ("qkv_b", "proj_b", "fc1_b", "fc2_b", "n1b", "n2b"):
            assert bool((w[b] != 0).all())
        assert float((w["n1w"] - 1).abs().min()) > 0 and float((w["n2w"] - 1).abs().min()) > 0
        assert float(inp["x"].mean(1).std()) > 1.0, "a per-row offset"
        assert all(bool((v != 0).all()) for v in inp["acc0"].values()), "every accumulator is preloaded"
        assert K.dims(c)["M"] % 256 != 0
    assert K.inputs(K.case_named("student"), dqkv_add=False)["dqkv_add"] is None


@pytest.mark.parametrize("c", BWD_CASES, ids=[c["name"] for c in BWD_CASES])
def test_without_dqkv_add_and_without_a_block_below(c):
    """the other variant of the inputs: no dqkv_add, no g_prev (block 0), fc2's bias gradient handed down by the block above"""
    inp = K.inputs(c, key=1, dqkv_add=False)
    route = K.default_routes(c, g2_bias_done=True, prev=False)
    rt, problems = K.audit(c, inp, K.emulate(c, inp, route=route), route)
    assert not problems and "g_prev" not in rt and rt["fc2_b"] == 0.0
    for name, r in rt.items():
        assert r < 1.0 if name in STORES16 else r <= 0.5, (c["name"], name, r)
    rt, _ = K.audit(c, inp, K.emulate(c, inp, route=K.default_routes(c, prev=False)), route)
    assert rt["fc2_b"] == float("inf"), "a bias gradient formed twice (handed down AND taken here) is seen"


# ---- the lean last block (devit_tail_fwd / devit_tail_bwd): tail_emulate under tail_audit
TAIL_STORES16 = STORES16 | {"kv", "ln1_tok", "q", "dq", "dkv", "dqkv_kv", "dln1_tok", "dln1/tok"}
TAIL_PLANT_CASES = ("tail_compacted", "tail_short", "tail_one_token")      # Da != D; N below a key tile; D != 384 (never a job)


@functools.lru_cache(maxsize=None)
def clean_tail(name):
    """(inputs, unmutated emulation, its audit) of a tail case: computed once, shared, left unchanged"""
    c = K.tail_case_named(name)
    inp = K.tail_inputs(c, c["ntok"])
    route = K.tail_routes(c, c["ntok"])
    bufs = K.tail_emulate(c, c["ntok"], inp)
    return inp, bufs, K.tail_audit(c, c["ntok"], inp, bufs, route)


@pytest.mark.parametrize("c", K.TAIL_CASES, ids=[c["name"] for c in K.TAIL_CASES])
def test_tail_emulation_passes_the_stage_audit(c):
    _, bufs, (rt, problems) = clean_tail(c["name"])
    print(" ".join(f"{k} {v:.3f}" for k, v in rt.items()))
    assert not problems, problems
    for name, r in rt.items():
        assert r < 1.0 if name in TAIL_STORES16 else r <= 0.5, (c["name"], name, r)
    # the whole list of the two calls, and every buffer they write is one the audit reads: nothing the lean block leaves in memory is unaudited
    assert list(rt) == list(K.TAIL_FWD_STAGES + K.TAIL_BWD_STAGES)
    assert set(K.tail_buffer_shapes(c, c["ntok"])) | {"x", "dx", "g2", "dx_in", "acc"} == set(bufs)
    assert set(bufs["acc"]) == set(K.ACC_NAMES)
    d = K.tail_dims(c, c["ntok"])
    for name, (rows, cols, is16) in K.tail_buffer_shapes(c, c["ntok"]).items():
        assert bufs[name].numel() == rows * cols and (bufs[name].dtype == K.BF16) == bool(is16), name
    assert d["M"] % 256 and d["T"] % 256, "every M and T is off the 256-row grid"


@pytest.mark.parametrize("mutate", sorted(K.TAIL_MUTATIONS))
def test_planted_tail_wiring_bug_is_seen(mutate):
    where = K.TAIL_MUTATIONS[mutate]
    for name in TAIL_PLANT_CASES:
        c = K.tail_case_named(name)
        nt = c["ntok"]
        inp = clean_tail(name)[0]
        route = K.tail_routes(c, nt, offered=mutate == "deferred_and_launched")
        rt, problems = K.tail_audit(c, nt, inp, K.tail_emulate(c, nt, inp, mutate=mutate, route=route), route)
        if mutate == "deferred_and_launched" and not route["kv_job"]:
            assert c["D"] != 384 and not problems and max(rt.values()) < 1.0, "no job is handed out: nothing to launch twice"
        elif where.startswith("pad_rows/"):
            assert where in problems, (name, mutate, problems)
        else:
            assert rt[where] >= 1.0, (name, mutate, where, rt[where])


def test_tail_mutation_table_lists_what_the_emulation_implements():
    import inspect
    import re
    src = inspect.getsource(K.tail_emulate)
    assert set(re.findall(r'mutate [!=]= "(\w+)"', src)) == set(K.TAIL_MUTATIONS)
    stages = set(K.TAIL_FWD_STAGES + K.TAIL_BWD_STAGES) | {"pad_rows/" + n for n in K.TAIL_PADDED_T + K.TAIL_PADDED_M}
    assert set(K.TAIL_MUTATIONS.values()) <= stages


def test_tail_routes_and_inputs_of_the_table():
    by = {v[0]: K.tail_routes(v[1], v[1]["ntok"], v[2], v[3]) for v in K.tail_variants()}
    assert [k for k, r in by.items() if r["kv_job"]] == ["tail_student/deferred"]
    assert all(r["branch"] == dict(wmode=False, fc2_bias="launch", fused=(False, False), prev=False) for r in by.values())
    assert K.tail_variants()[3][3], "tail_one_token is offered a slot and must not take it"
    shapes = {c["name"]: (c["B"], c["N"], c["ntok"], c["D"], c["heads"], c["hidden"]) for c in K.TAIL_CASES}
    assert shapes == {"tail_student": (3, 198, 2, 384, 6, 1536), "tail_one_token": (2, 197, 1, 256, 4, 512), "tail_compacted": (3, 51, 2, 384, 4, 640),
                      "tail_short": (4, 6, 2, 384, 6, 768), "tail_two_tiles": (130, 6, 2, 384, 6, 768), "tail_wide_tokens": (2, 198, 40, 384, 6, 1536)}
    for c in K.TAIL_CASES:
        inp = clean_tail(c["name"])[0]
        assert all(bool((v != 0).all()) for v in inp["acc0"].values()), "every accumulator is preloaded"
        assert inp["g2"].shape[0] == c["B"] * c["ntok"] and not torch.equal(inp["w"]["dp1"], inp["w"]["dp2"])
        assert bool((inp["w"]["head_gate"] == 0).any()) and bool((inp["w"]["neuron_gate"] == 0).any())


def test_tail_arena_sees_a_write_outside_an_extent():
    """the arena of the GPU test, on the host: slots at the library's sizes, clean when only the stated extents are written, and a byte behind an
    extent, or in a guard, is named"""
    c = K.tail_case_named("tail_compacted")
    ar = K.tail_arena("cpu", c, c["ntok"])
    acts, bwd = K.tail_library_sizes(3, 51, 2, 384, 256, 640, K.SAVE)
    assert ar.sizes["kv"] == acts["qkv"] and ar.sizes["dkv"] == bwd["dkv"] and ar.adr("att") is None
    for name, e in ar.extents.items():
        ar.mem[ar.off[name]:ar.off[name] + e] = 0
    assert ar.written_outside() == []
    slack = [n for n, e in ar.extents.items() if e < ar.sizes[n]]
    assert slack, "a slot with bytes beyond its extent"
    ar.mem[ar.off[slack[0]] + ar.extents[slack[0]]] = 0
    ar.mem[0] = 0
    ar.mem[-1] = 0
    assert ar.written_outside() == ["extent/" + slack[0], "guard/front", "guard/back"]


# ---- host-only statements about the library
@pytest.mark.parametrize("c", K.CASES, ids=[c["name"] for c in K.CASES])
def test_reported_sizes_hold_the_stated_extents(c):
    """devit_block_acts_sizes / devit_block_bwd_sizes against the extents the header words: at least the extent, 256-aligned, exactly 0 for what
    the flags leave out"""
    acts, bwd = K.library_sizes(c)
    for got, want in ((acts, K.act_extents(c)), (bwd, K.bwd_extents(c))):
        assert set(got) == set(want)
        for name, n in want.items():
            assert got[name] % 256 == 0 and got[name] >= n, (c["name"], name, got[name], n)
            assert (got[name] == 0) == (n == 0), (c["name"], name, got[name], n)
            assert got[name] < n + 256, (c["name"], name, "more than one alignment step over the stated extent")
    from devit_amd import _lib as L
    d = K.dims(c)
    assert L.load().devit_layernorm_bwd_workspace(d["M"], d["D"]) == K.bwd_extents(c)["lnws"]
    assert L.load().devit_colsum_workspace(d["Mp"], d["D"]) == 64 * d["D"] * 4, "the figure default_routes() restates"


@pytest.mark.parametrize("dims", K.TAIL_SIZE_CASES, ids=["x".join(map(str, d)) for d in K.TAIL_SIZE_CASES])
@pytest.mark.parametrize("save", (1, 0))
def test_reported_tail_sizes_hold_the_stated_extents(dims, save):
    """devit_tail_acts_sizes / devit_tail_bwd_sizes, as for the block: at least the extent the header words (pad rows of T = B ntok and of M counted),
    256-aligned, less than one alignment step over, exactly 0 for what the flags leave out (and for `att`, which the lean block never has)"""
    acts, bwd = K.tail_library_sizes(*dims, K.SAVE if save else 0)
    want_a, want_b = K.tail_extents(*dims, save)
    B, N, ntok, D, Da, Hd = dims
    assert want_a["ln2"] == K.pad_rows(B * ntok) * D * 2 and want_a["qkv"] == K.pad_rows(B * N) * 2 * Da * 2
    for got, want in ((acts, want_a), (bwd, want_b)):
        assert set(got) == set(want)
        for name, n in want.items():
            assert got[name] % 256 == 0 and n <= got[name] < n + 256, (dims, name, got[name], n)
            assert (got[name] == 0) == (n == 0), (dims, name, got[name], n)


def test_routes_of_the_table():
    """the branches the table is there for, from the restated rule"""
    r = {c["name"]: K.default_routes(c) for c in BWD_CASES}
    assert r["student"]["wmode"] and r["student"]["fc2_bias"] == "colsum"
    assert r["compacted"]["wmode"] and r["compacted"]["fc2_bias"] == "launch"
    assert not r["wide"]["wmode"] and r["wide"]["fc2_bias"] == "launch"
    assert r["short"]["wmode"] and r["short"]["fc2_bias"] == "launch"
    assert not K.default_routes(K.case_named("compacted"), {"DEVIT_WGRADFR": "0"})["wmode"]
    assert K.qkv_extra(K.case_named("compacted")) == 205 and K.qkv_extra(K.case_named("student")) == 128


def fake(name):
    return 0x100000 * (1 + sum(ord(ch) for ch in name) % 97)


@pytest.mark.parametrize("name,case,change,entry,code,words", K.REFUSALS, ids=[r[0] for r in K.REFUSALS])
def test_entry_points_refuse_before_anything_is_launched(name, case, change, entry, code, words):
    """with addresses that are not memory: a check that came after a launch (or a dereference) could not return its own code here"""
    rc, msg = K.refused(case, change, entry, fake)
    assert rc == code and words in msg, (name, rc, msg)


def test_sizes_functions_refuse():
    for name, rc, msg, code, words in K.sizes_refusals():
        assert rc == code and words in msg, (name, rc, msg)
