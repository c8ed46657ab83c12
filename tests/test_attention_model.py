"""The attention error model itself under test (tests/_attn_model.py), on a machine without a GPU: on the fixed inputs the GPU tests use,
a plain-torch emulation of the roundings csrc/attention.hip documents must stay inside every elementwise bound and within the gain
bar, and planted bugs must break them.  This is what shows that the bounds the GPU tests hold the kernels to can fail."""
import pytest
import torch

import _attn_model as A

SCALE = 0.125


def _case(B, N, H, regime, gated, with_add, gate=None, mutate=None, nonzero=False):
    inp = A.make_inputs(B, N, H, regime)
    if gate is None and gated:
        gate = A.gate_mix(H, nonzero)
    q, k, v, do, ad = A.split_packed(inp["qkv"], B, N, H, inp["dout"], inp["add"] if with_add else None)
    ref, bnd = A.bounds(q, k, v, gate, SCALE, do, ad)
    emu = A.emulate(q, k, v, gate, SCALE, do, ad, mutate=mutate)
    return ref, bnd, emu


# flat / unit / peaked over N in {1, 17, 193, 198, 208}: a subset of _attn_model.packed_cases()
CASES = [c for c in A.packed_cases() if c[1] in (1, 17, 193, 198, 208)]


@pytest.mark.parametrize("B,N,H,regime,gated,with_add", CASES)
def test_emulation_stays_inside_every_bound(B, N, H, regime, gated, with_add):
    ref, bnd, emu = _case(B, N, H, regime, gated, with_add)
    res = {n: A.ratio(emu[n], ref[n], bnd[n]) for n in ("O", "lse", "dQ", "dK", "dV")}
    print(res)
    assert all(x < 1.0 for x in res.values()), res
    if gated and H >= 3:                     # a head gated off: bound exactly 0, output exactly 0
        assert float(bnd["O"][:, 2].abs().max()) == 0.0 and float(emu["O"][:, 2].abs().max()) == 0.0
        if not with_add:
            for n in ("dQ", "dK", "dV"):
                assert float(bnd[n][:, 2].abs().max()) == 0.0 and float(emu[n][:, 2].abs().max()) == 0.0, n


@pytest.mark.parametrize("regime", ["unit", "flat"])
def test_emulation_gain(regime):
    """per head and per output |slope - 1| <= 2^-9; >= 10^4 elements per head"""
    B, N, H = 4, 198, 6
    ref, bnd, emu = _case(B, N, H, regime, True, False, nonzero=True)
    assert B * N * 64 >= 10 ** 4
    for n in ("O", "dQ", "dK", "dV"):
        s = A.slope(emu[n], ref[n])
        print(n, (s - 1).abs().max().item())
        assert bool(((s - 1).abs() <= A.SLOPE_BAR).all()), (n, s)
    scaled = A.slope(emu["dQ"] * 1.01, ref["dQ"])           # a 1 % gain error: below every max-error bound, not below this bar
    assert A.ratio(emu["dQ"] * 1.01, ref["dQ"], bnd["dQ"]) < 1.0
    assert bool(((scaled - 1).abs() > A.SLOPE_BAR).all()), scaled


@pytest.mark.parametrize("regime", ["unit", "flat"])
@pytest.mark.parametrize("mutate,broken", [("dq_drops_last_key", "dQ"), ("dk_drops_ds_tile", "dK"), ("dv_drops_p_tile", "dV"),
                                           ("delta_from_pregate_out", "dQ")])
def test_planted_bugs_break_a_bound(regime, mutate, broken):
    B, N, H = 2, 198, 6
    gate = torch.full((H,), 0.5) if mutate == "delta_from_pregate_out" else None
    ref, bnd, emu = _case(B, N, H, regime, False, False, gate=gate, mutate=mutate)
    res = {n: A.ratio(emu[n], ref[n], bnd[n]) for n in ("O", "lse", "dQ", "dK", "dV")}
    print(mutate, regime, res)
    assert res[broken] > 1.0, res
    for n in ("O", "lse"):                   # the forward is not mutated
        assert res[n] < 1.0, res


def test_delta_from_pregate_out_with_gate_zero_breaks_the_exact_zero_rule():
    B, N, H = 2, 198, 6
    gate = torch.zeros(H)
    ref, bnd, emu = _case(B, N, H, "unit", False, False, gate=gate, mutate="delta_from_pregate_out")
    assert float(bnd["dQ"].abs().max()) == 0.0
    assert A.ratio(emu["dQ"], ref["dQ"], bnd["dQ"]) == float("inf")
    ok = _case(B, N, H, "unit", False, False, gate=gate)[2]
    assert A.ratio(ok["dQ"], ref["dQ"], bnd["dQ"]) == 0.0


@pytest.mark.parametrize("N", [208, 198, 193, 64, 17])
def test_routing_inputs_saturate_the_softmax(N):
    """the matching score is 128, every other one <= 72: P is one-hot to 1e-22 and the emulation returns g V[pi(i)] exactly"""
    B, H = 2, 2
    inp = A.routing_inputs(B, N, H)
    assert inp["max_other"] <= 72
    gate = torch.tensor([2.0, 0.5])
    q, k, v, do, _ = A.split_packed(inp["qkv"], B, N, H, inp["dout"])
    ref, bnd = A.bounds(q, k, v, gate, SCALE, do)
    emu = A.emulate(q, k, v, gate, SCALE, do)
    want = gate.double().view(1, H, 1, 1) * torch.gather(v, 2, inp["perm"][..., None].expand(B, H, N, 64))
    assert torch.equal(emu["O"], want)
    assert float((ref["P"].amax(-1) - 1).abs().max()) < 1e-20
    for n in ("O", "lse", "dQ", "dK", "dV"):
        assert A.ratio(emu[n], ref[n], bnd[n]) < 1.0, n


def test_f16_forward_emulation_inside_its_bound():
    for B, N, H, regime in ((2, 198, 6, "peaked"), (2, 193, 12, "unit")):
        inp = A.make_inputs(B, N, H, regime, dtype=A.F16)
        q, k, v, _, _ = A.split_packed(inp["qkv"], B, N, H)
        gate = A.gate_mix(H)
        ref, bnd = A.bounds(q, k, v, gate, SCALE, u=A.U_F16, f16=True)
        emu = A.emulate(q, k, v, gate, SCALE, f16=True)
        res = {n: A.ratio(emu[n], ref[n], bnd[n]) for n in ("O", "lse")}
        print(res)
        assert all(x < 1.0 for x in res.values()), res


@pytest.mark.parametrize("std", [0.25, 1.0])
def test_relation_gradient_bound(std):
    """The bound tests/test_gpu_kernels.py::test_relation_loss holds the relation-loss gradient to, on that test's inputs: an fp32 restatement of
    the launches stays inside it, one that loses the transposed half of S = G + G^T does not.  At unit scale the first two terms alone
    (u (|S||F| + |dF|) + e32 256 |S||F|) are exceeded more than tenfold by the honest fp32 restatement: the four exponentials of
    rel_grad_kernel cancel there, which is what the E_249 term of relation_bounds() accounts for."""
    B, N, Ds, Dt = 3, 198, 128, 256

    def rnd(shape, seed):
        g = torch.Generator(device="cpu").manual_seed(seed)
        return (torch.randn(shape, generator=g) * std).to(A.BF16)

    s, t = rnd((B * N, 3 * Ds), 1), rnd((B * N, 3 * Dt), 2)
    for j, w in enumerate((0.2 / 12, 0.1 / 12, 0.3 / 12)):
        fs = s[:, j * Ds:(j + 1) * Ds].double().view(B, N, Ds)
        ft = t[:, j * Dt:(j + 1) * Dt].double().view(B, N, Dt)
        want, bound, S = A.relation_bounds(fs, ft, w, 64, 64)
        good = A.ratio(A.relation_emulate(fs, ft, w, 64, 64), want, bound)
        bad = A.ratio(A.relation_emulate(fs, ft, w, 64, 64, mutate=True), want, bound)
        print(std, j, good, bad)
        assert good < 1.0 and bad > 1.0, (std, j, good, bad)
        if std == 1.0:
            SF = S.abs() @ fs.abs()
            first_two = A.U_BF16 * (SF + want.abs()) + A.E32 * 256 * SF
            assert A.ratio(A.relation_emulate(fs, ft, w, 64, 64), want, first_two) > 10.0
