"""tests/_hid_model.py held on the CPU: the float64 restatement of cal_hid_relation_loss against the reference's golden step and against torch
autograd, the per-element error model against an honest emulation of the kernel sequence (which must sit inside it) and against a lower-precision
one (which must not), and the --hid-gama flag."""
import pytest
import torch

import _hid_model as HM
from _hid_model import F64


def _case(B, N, Ds, Dt, regime):
    return HM.inputs(B, N, Ds, Ds if regime == "same" else Dt, regime)


def test_restatement_vs_golden(golden):
    """the reference's own function on CPU fp32 (tests/golden/make_golden_hid.py): loss and both student gradients to fp32 agreement -- a few fp32
    roundings of the loss (its sum has 98 terms per pair), 1e-5 of the largest gradient element"""
    g = golden("hid_relation")
    stu, tea = HM.golden_inputs()
    loss, grads = HM.cal(stu, tea)
    assert abs(float(loss) - float(g["loss"])) <= 2e-6 * abs(float(loss))
    for i, dh in enumerate(grads):
        ref = torch.from_numpy(g[f"grad_s{i}"]).to(F64)
        assert float((dh - ref).abs().max()) <= 1e-5 * float(ref.abs().max()), i


@pytest.mark.parametrize("regime", HM.REGIMES)
def test_restatement_vs_autograd(regime):
    """the analytic backward against torch autograd of the definition, both in float64: 1e-13 of the largest element (float64 sums of a few
    hundred terms; measured 4e-16 absolute at unit scale)"""
    s, t = _case(2, 6, 64, 128, regime)
    s64 = s.to(F64).requires_grad_(True)
    loss = HM.autograd_loss([s64], [t.to(F64)])
    loss.backward()
    r = HM.restate(s, t)
    assert abs(float(r["loss"]) - float(loss.detach())) <= 1e-13 * abs(float(loss.detach()))
    # the scale of the two terms that cancel in dh = inv (dh^ - h^ (h^ . dh^)): with a common offset dh^ is nearly parallel to h^
    scale = float((r["inv_s"][..., None] * (r["dhn"].abs() + r["hs"].abs() * r["p"].abs())).max())
    assert float((r["dh"] - s64.grad).abs().max()) <= 1e-13 * scale
    if regime == "same":
        assert float(r["loss"]) == 0.0 and float(r["dh"].abs().max()) == 0.0


def test_list_form_divides_by_the_number_of_pairs():
    stu, tea = HM.golden_inputs()
    both, _ = HM.cal(stu, tea)
    one = [HM.cal([s], [t])[0] for s, t in zip(stu, tea)]
    assert abs(float(both) - float(sum(one)) / 2) <= 1e-15
    assert abs(float(HM.autograd_loss([x.to(F64) for x in stu], [x.to(F64) for x in tea])) - float(both)) <= 1e-15


@pytest.mark.parametrize("regime", HM.REGIMES)
@pytest.mark.parametrize("B,N,Ds,Dt", HM.CASES)
def test_emulation_inside_bounds(B, N, Ds, Dt, regime):
    """fp32 arithmetic with ONE bf16 rounding of h^ and of S stays inside the per-element bounds at every shape and regime of the GPU test"""
    s, t = _case(B, N, Ds, Dt, regime)
    r, bnd = HM.bounds(s, t, layers=1, upstream=0.5)
    e = HM.emulate(s, t, layers=1, upstream=0.5)
    worst = {k: HM.ratio(e[k], r[k], bnd[k]) for k in ("hs", "inv_s", "loss", "S", "dh")}
    assert all(v <= 1.0 for v in worst.values()), worst
    assert bool(torch.isfinite(e["dh"]).all()) and bool(torch.isfinite(e["loss"]))
    if regime == "zero_row":
        assert float(e["hs"][0, N // 2].abs().max()) == 0.0 and float(e["inv_s"][0, N // 2]) == pytest.approx(1e12, rel=1e-6)
    if regime == "same":
        assert float(e["loss"]) == 0.0 and float(e["dh"].abs().max()) == 0.0


def test_bounds_can_fail():
    """Grams whose running sums are kept in bf16 (every addition rounded to 8 bits) leave the bounds of everything computed from them: the model
    is not wide enough to hide a lower-precision accumulation"""
    s, t = HM.inputs(2, 6, 384, 768, "unit")
    r, bnd = HM.bounds(s, t)
    ok, low = HM.emulate(s, t), HM.emulate(s, t, variant="gram_bf16")
    for k in ("loss", "S", "dh"):
        assert HM.ratio(ok[k], r[k], bnd[k]) <= 1.0, k
    for k in ("loss", "S"):          # (dh's bound also carries the worst case of the projection's two cancelling terms: the variant stays inside it)
        assert HM.ratio(low[k], r[k], bnd[k]) > 1.0, k
    assert HM.ratio(low["hs"], r["hs"], bnd["hs"]) <= 1.0            # (the variant changes nothing before the Grams)


def test_scale_invariance_of_the_restatement():
    s, t = HM.inputs(2, 6, 64, 128, "unit")
    a, b = HM.restate(s, t), HM.restate(s.to(F64) * 1e3, t.to(F64) * 1e-3)
    assert abs(float(a["loss"]) - float(b["loss"])) <= 1e-12 * float(a["loss"])
    assert float((a["dh"] - b["dh"] * 1e3).abs().max()) <= 1e-10 * float(a["dh"].abs().max())


def test_cli_hid_gama_flag():
    """--hid-gama: default 0, any value >= 0 accepted, a negative one refused by the parser"""
    import distill_sub
    p = distill_sub.get_args_parser()
    assert p.parse_args([]).hid_gama == 0.0
    assert p.parse_args(["--hid-gama", "0.3"]).hid_gama == pytest.approx(0.3)
    for bad in ("-0.1", "nan"):
        with pytest.raises(SystemExit):
            p.parse_args(["--hid-gama", bad])


def test_engine_refuses_negative_hid_gama():
    from devit_amd import engine
    with pytest.raises(ValueError):
        engine.distill_forward(torch.nn.Identity(), torch.nn.Identity(), None, None, hid_gama=-1.0)
