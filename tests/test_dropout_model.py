"""The dropout models themselves under test, on a machine without a GPU: tests/_drop_model.py (the three kernels of csrc/dropout.hip) and the
keep / s arguments of tests/_attn_model.py (the *_drop kernels of csrc/attention.hip).  On the cases the GPU tests use, a restatement of
each kernel's roundings and index arithmetic stays inside every bound, every planted bug breaks the bound of its named case and output,
the float64 statements equal torch autograd, and the case table reaches the seams it was built for."""
import math

import numpy as np
import pytest
import torch

import _attn_model as A
import _drop_model as M
import _philox as PH

SCALE = 0.125
F64 = torch.float64


# ------------------------------------------------------------------------------------------ csrc/dropout.hip
@pytest.mark.parametrize("name", list(M.CASES))
def test_emulation_is_inside_every_bound(name):
    res = M.run_emulation(M.CASES[name])
    print(name, res)
    assert res and all(x < 1.0 for x in res.values()), res


@pytest.mark.parametrize("mutate,name,broken,untouched", [(m, n, b, u) for m, rows in M.PLANTED.items() for n, b, u in rows])
def test_planted_index_bugs_break_their_output(mutate, name, broken, untouched):
    res = M.run_emulation(M.CASES[name], mutate)
    print(mutate, name, res)
    assert set(broken) | set(untouched) == set(res)
    for n in broken:
        assert res[n] >= 1.0, (n, res)
    for n in untouched:
        assert res[n] < 1.0, (n, res)


def test_every_mutation_is_planted():
    assert set(M.PLANTED) == set(M.MUTATIONS)


@pytest.mark.parametrize("name", list(M.CASES))
def test_every_case_keeps_and_drops(name):
    keep = M.keep_of(M.CASES[name])
    assert 0 < int(keep.sum()) < keep.numel(), name
    if keep.shape[0] > 1:            # ... and no two rows alike (a row index that does not reach the counter)
        assert len({bytes(r) for r in keep.numpy().astype(np.uint8)[:64]}) == min(keep.shape[0], 64)


def test_the_case_table_reaches_its_seams():
    """computed from the launch arithmetic of dropout.hip as _drop_model.grid() restates it, not asserted from the case's name"""
    C = M.CASES
    # the high counter word: rows 1 and 2 of the 2^34 cases
    for n in ("mask/hi-2p34", "mask/hi-2p34+4", "apply/bf16-hi", "apply/f32-hi"):
        c = C[n]
        assert M.high_word_max(c) == 2 and (1 * c["pitch"]) >> 34 == 1, n
    assert all(M.high_word_max(c) == 0 for n, c in C.items() if c["kernel"] != "residual" and "hi" not in n)
    # a second trip of every grid-stride loop
    g = M.grid(C["mask/stride"])
    assert g["gx"] == M.MASK_GRID and g["trips"] == 2 and 1025 * 1025 - M.MASK_GRID * M.MASK_WG == 2049
    for n, trips, gy in (("apply/bf16-1029x520-sum", 3, 128), ("apply/f32-1029x260-sum", 3, 128), ("apply/bf16-4101x520", 2, 1024),
                         ("residual/4101x260-rps3", 2, 1024), ("residual/4101x260-rps198", 2, 1024)):
        g = M.grid(C[n])
        assert (g["gx"], g["gy"], g["trips"]) == (2, gy, trips), (n, g)      # 65 lanes: a second workgroup column with one live lane
        assert C[n]["rows"] % (gy * M.RY) != 0 and C[n]["rows"] % M.RY != 0                 # the last trip and the last workgroup are ragged
    # cols % 4 in 1, 2, 3, tight and wide pitch
    seen = {(c["cols"] % 4, c["pitch"] == M.ceil4(c["cols"])) for c in M.MASK_CASES if c["rows"] == 5}
    assert seen == {(k, t) for k in (1, 2, 3) for t in (True, False)}
    assert any(c["seed"] >> 32 for c in M.MASK_CASES) and {c["p"] for c in M.APPLY_CASES} == {0.1, 0.5} == {c["p"] for c in M.RESIDUAL_CASES}
    for dt in (M.BF16, M.F32):
        assert any(c["ld"] > c["cols"] and c["colsum"] and c["dtype"] == dt for c in M.APPLY_CASES), dt
    assert {(c["rowscale"], c["in_place"]) for c in M.RESIDUAL_CASES} >= {("zeros", False), ("zeros", True), (None, False), (None, True)}
    assert {c["rps"] for c in M.RESIDUAL_CASES} >= {3, 198}


def test_a_64_bit_seed_uses_both_key_words():
    c = M.CASES["mask/seed64"]
    lo = dict(c, seed=c["seed"] & 0xFFFFFFFF)
    assert not torch.equal(M.keep_of(c), M.keep_of(lo))
    assert torch.equal(M.emulate_mask(c), M.keep_of(c))


def test_dropout_statements_equal_autograd():
    """y = (h + b) keep s: the apply statement on dY is dh, its column sums are db; out = x + rs keep s y is the residual statement"""
    c = M.CASES["apply/f32-ld"]
    inp = M.inputs(c)
    keep, s = M.keep_of(c), M.thr_s(c["p"])[1]
    dy = inp["x"][:, :c["cols"]].to(F64)
    h = torch.zeros_like(dy, requires_grad=True)
    b = torch.zeros(c["cols"], dtype=F64, requires_grad=True)
    ((h + b) * keep * s).backward(dy)
    stored, colsum, _ = M.apply_statement(c, inp)
    # the statement's stored value is the fp32 product: within 2^-24 of the float64 one
    assert float((stored.to(F64) - h.grad).abs().max()) <= M.U24 * float(h.grad.abs().max())
    assert float((colsum - inp["colsum0"].to(F64) - stored.to(F64).sum(0)).abs().max()) <= 1e-12
    assert float((b.grad - h.grad.sum(0)).abs().max()) <= 1e-12 * float(b.grad.abs().max())
    c = M.CASES["residual/4101x260-rps3"]
    inp = M.inputs(c)
    want, _, exact = M.residual_statement(c, inp)
    rs = inp["rowscale"].to(F64).repeat_interleave(c["rps"])[:, None]
    ref = inp["x"].to(F64) + rs * (M.keep_of(c) * inp["y"].to(F64) * M.thr_s(c["p"])[1])
    assert float((want - ref).abs().max()) <= 1e-12 * float(ref.abs().max())
    assert torch.equal(want[exact], inp["x"].to(F64)[exact])


# ------------------------------------------------------------------------------------------ the *_drop kernels of csrc/attention.hip
def _attn_case(B, N, H, regime, gated, with_add, p, block, mutate=None, keep_bwd=None, gate=None):
    inp = A.make_inputs(B, N, H, regime)
    if gate is None and gated:
        gate = A.gate_mix(H)
    thr, s = A.drop_params(p)
    keep = A.attn_keep(A.DROP_SEED, block, thr, B, H, N)
    q, k, v, do, ad = A.split_packed(inp["qkv"], B, N, H, inp["dout"], inp["add"] if with_add else None)
    ref, bnd = A.bounds(q, k, v, gate, SCALE, do, ad, keep=keep, s=s)
    emu = A.emulate(q, k, v, gate, SCALE, do, ad, mutate=mutate, keep=keep, s=s, keep_bwd=keep_bwd)
    return ref, bnd, emu, {n: A.ratio(emu[n], ref[n], bnd[n]) for n in ("O", "lse", "dQ", "dK", "dV")}


@pytest.mark.parametrize("B,N,H,regime,gated,with_add,p,block", A.DROP_CASES)
def test_dropped_attention_emulation_is_inside_every_bound(B, N, H, regime, gated, with_add, p, block):
    ref, bnd, emu, res = _attn_case(B, N, H, regime, gated, with_add, p, block)
    print(res)
    assert all(x < 1.0 for x in res.values()), res
    if gated and H >= 3:                     # a head gated off: bound exactly 0, output exactly 0
        assert float(bnd["O"][:, 2].abs().max()) == 0.0 and float(emu["O"][:, 2].abs().max()) == 0.0
        if not with_add:
            for n in ("dQ", "dK", "dV"):
                assert float(bnd[n][:, 2].abs().max()) == 0.0 and float(emu[n][:, 2].abs().max()) == 0.0, n


@pytest.mark.parametrize("p", [0.9])
def test_dropped_attention_emulation_at_a_high_rate(p):
    for B, N, H, regime in ((2, 198, 6, "unit"), (2, 193, 3, "peaked"), (1, 208, 1, "flat")):
        res = _attn_case(B, N, H, regime, True, True, p, 2)[3]
        print(regime, res)
        assert all(x < 1.0 for x in res.values()), res


def test_the_drop_cases_cover_what_they_claim():
    assert {c[1] for c in A.DROP_CASES} == {198, 208, 193, 65, 17, 5, 1} and {c[3] for c in A.DROP_CASES} == set(A.REGIMES)
    assert {c[6] for c in A.DROP_CASES} == {0.1, 0.5} and len({c[7] for c in A.DROP_CASES}) == 2
    assert {c[5] for c in A.DROP_CASES} == {True, False} and any(c[4] and c[2] >= 3 for c in A.DROP_CASES)
    assert {c[0] for c in A.DROP_CASES} == {1, 2} and min(c[2] for c in A.DROP_CASES) == 1 and max(c[2] for c in A.DROP_CASES) == 6
    for B, N, H, _, _, _, p, block in A.DROP_CASES:
        if N >= 5:
            keep = A.attn_keep(A.DROP_SEED, block, A.drop_params(p)[0], B, H, N)
            assert 0 < int(keep.sum()) < keep.numel()


# planted bug -> (case, outputs it must break, outputs that must stay inside)
_BIG = (2, 198, 6, "unit", False, False, 0.1, 4)
ATTN_PLANTED = [
    ("drop_bwd_mask_other_block", _BIG, ("dQ", "dK", "dV"), ("O", "lse")),
    ("drop_bwd_mask_other_block", (2, 193, 3, "flat", False, True, 0.5, 1), ("dQ", "dK", "dV"), ("O", "lse")),
    ("drop_bwd_mask_pitch_n", _BIG, ("dQ", "dK", "dV"), ("O", "lse")),
    ("drop_bwd_mask_pitch_n", (1, 5, 2, "unit", False, False, 0.5, 4), ("dQ", "dK", "dV"), ("O", "lse")),
    ("drop_lse_of_dropped_row", _BIG, ("lse", "O"), ()),
    ("drop_delta_from_undropped_out", _BIG, ("dQ", "dK"), ("O", "lse", "dV")),
    ("drop_dv_scaled_twice", _BIG, ("dV",), ("O", "lse", "dQ", "dK")),
    ("drop_quad_trade_transposed", _BIG, ("dQ", "dK", "dV"), ("O", "lse")),
    ("drop_quad_trade_transposed", (2, 17, 2, "flat", False, False, 0.5, 1), ("dQ", "dK", "dV"), ("O", "lse")),
]


@pytest.mark.parametrize("mutate,case,broken,inside", ATTN_PLANTED)
def test_planted_attention_bugs_break_their_output(mutate, case, broken, inside):
    B, N, H, regime, gated, with_add, p, block = case
    thr = A.drop_params(p)[0]
    keep_bwd = None
    if mutate == "drop_bwd_mask_other_block":
        keep_bwd = A.attn_keep(A.DROP_SEED, block + 1, thr, B, H, N)
    if mutate == "drop_bwd_mask_pitch_n":
        assert N % 4 != 0
        keep_bwd = A.attn_keep(A.DROP_SEED, block, thr, B, H, N, pitch=N)
    res = _attn_case(*case, mutate=mutate, keep_bwd=keep_bwd)[3]
    print(mutate, case, res)
    for n in broken:
        assert res[n] >= 1.0, (n, res)
    for n in inside:
        assert res[n] < 1.0, (n, res)


def test_every_attention_mutation_is_planted():
    assert {m for m, *_ in ATTN_PLANTED} == {m for m in A.MUTATIONS if m.startswith("drop_")}


def test_a_wrong_backward_mask_breaks_the_exact_zero_rule_nowhere_else():
    """gate 0: the bounds are exactly 0 and so is every output, whichever mask the backward takes (nothing is hidden by a zero bound
    that is not zero)"""
    B, N, H, p, block = 1, 17, 2, 0.5, 1
    ref, bnd, emu, res = _attn_case(B, N, H, "unit", False, False, p, block, gate=torch.zeros(H))
    assert all(float(bnd[n].abs().max()) == 0.0 for n in ("O", "dQ", "dK", "dV")) and all(res[n] == 0.0 for n in ("O", "dQ", "dK", "dV"))


@pytest.mark.parametrize("B,N,H,with_add", [(2, 17, 3, True), (1, 65, 2, False), (1, 5, 1, True)])
def test_the_dropped_statement_equals_autograd(B, N, H, with_add):
    inp = A.make_inputs(B, N, H, "unit")
    thr, s = A.drop_params(0.5)
    keep = A.attn_keep(A.DROP_SEED, 3, thr, B, H, N)
    gate = A.gate_mix(H)
    q, k, v, do, ad = A.split_packed(inp["qkv"], B, N, H, inp["dout"], inp["add"] if with_add else None)
    ref = A.reference(q, k, v, gate, SCALE, do, ad, keep=keep, s=s)
    qa, ka, va = (t.clone().requires_grad_(True) for t in (q, k, v))
    P = torch.softmax(SCALE * (qa @ ka.transpose(-1, -2)), -1) * (keep.to(F64) * s)
    O = gate.to(F64).view(1, H, 1, 1) * (P @ va)
    O.backward(do)
    for n, got, a in (("dQ", qa.grad, 0), ("dK", ka.grad, 1), ("dV", va.grad, 2)):
        want = ref[n] - (ad[a] if with_add else 0.0)
        assert float((got - want).abs().max()) <= 1e-12 * max(float(want.abs().max()), 1.0), n
    assert float((O.detach() - ref["O"]).abs().max()) <= 1e-12 * float(ref["O"].abs().max())
    assert float((ref["lse"] - torch.logsumexp(SCALE * (q @ k.transpose(-1, -2)), -1)).abs().max()) == 0.0


@pytest.mark.parametrize("B,N,H,regime", [(2, 198, 6, "unit"), (2, 17, 2, "peaked")])
def test_keep_none_is_what_the_functions_were(B, N, H, regime):
    """keep=None takes none of the dropout lines: the plain statement restated here gives the same bits, and so does an all-kept mask
    with s = 1 in reference() and emulate() (multiplications by exactly 1); only the bounds of the dropped form are wider"""
    inp = A.make_inputs(B, N, H, regime)
    gate = A.gate_mix(H)
    q, k, v, do, ad = A.split_packed(inp["qkv"], B, N, H, inp["dout"], inp["add"])
    ref, bnd = A.bounds(q, k, v, gate, SCALE, do, ad)
    g = gate.to(F64).view(1, H, 1, 1)
    S = SCALE * (q @ k.transpose(-1, -2))
    lse = torch.logsumexp(S, -1)
    P = torch.exp(S - lse[..., None])
    O = g * (P @ v)
    dS = P * (g * (do @ v.transpose(-1, -2)) - (do * O).sum(-1, keepdim=True))
    plain = dict(O=O, lse=lse, dS=dS, dQ=SCALE * (dS @ k) + ad[0], dK=SCALE * (dS.transpose(-1, -2) @ q) + ad[1],
                 dV=g * (P.transpose(-1, -2) @ do) + ad[2])
    for n, t in plain.items():
        assert torch.equal(ref[n], t), n
    assert "Pd" not in ref
    ones = torch.ones((B, H, N, N), dtype=torch.bool)
    ref1, bnd1 = A.bounds(q, k, v, gate, SCALE, do, ad, keep=ones, s=1.0)
    emu, emu1 = A.emulate(q, k, v, gate, SCALE, do, ad), A.emulate(q, k, v, gate, SCALE, do, ad, keep=ones, s=1.0)
    for n in ("O", "lse", "dQ", "dK", "dV"):
        assert torch.equal(ref[n], ref1[n]) and torch.equal(emu[n], emu1[n]), n
        assert bool((bnd1[n] >= bnd[n]).all()), n
    assert math.isfinite(float(bnd["dQ"].max()))
