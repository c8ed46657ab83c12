"""tests/_qkvce_model.py held on the CPU: the float64 restatement of cal_qkv_loss / cal_qkv_loss2 / soft_cross_entropy against the reference's golden
run and against torch autograd of the definition, the per-element error model against an honest fp32 emulation of the kernel sequence (which must
sit inside it) and against four wrong kernels (each of which must leave it somewhere), the chunk map of the reference's `.view`, and the flags."""
import pytest
import torch

import _qkvce_model as QM
from _qkvce_model import F64


def _case(B, N, Ds, Dt, regime):
    return QM.inputs(B, N, Ds, Ds if regime == "same" else Dt, regime)


@pytest.mark.parametrize("name,cross", [("self", False), ("cross", True)])
@pytest.mark.parametrize("npairs", [1, 2])
def test_restatement_vs_golden(golden, name, cross, npairs):
    """The reference's own functions on CPU fp32 (tests/golden/make_golden_qkvce.py), layout "view".  The bar is the roundoff of THAT fp32 run: a Gram
    entry is an fp32 sum of D products and a softmax row an fp32 sum of N exponentials, so an argument of an exponential is off by at most
    2^-23 (D + 2 N + 16) max|Z| -- D = 192 (the teacher's), N = 5 -- which is the relative error of every probability, hence of the loss (relative)
    and of the gradient (relative to its largest element; the gradient is linear in the probabilities)."""
    g = golden("qkvce")
    stu, tea = QM.golden_inputs()
    stu, tea = stu[:npairs], tea[:npairs]
    loss, grads = QM.cal(stu, tea, cross, "view")
    zmax = max(float((QM.rows(QM.pack(m).to(F64), i, "view") @ QM.rows(QM.pack(m).to(F64), j, "view").transpose(1, 2)).abs().max()) / 8.0
               for m in stu + tea for i in range(3) for j in range(3))
    bar = 2.0 ** -23 * (192 + 2 * 5 + 16) * zmax
    ref = float(g[f"{name}{npairs}_loss"])
    print(f"{name}{npairs}: loss {float(loss):.9f} golden {ref:.9f} rel {abs(float(loss) - ref) / ref:.2e} bar {bar:.2e}")
    assert abs(float(loss) - ref) <= bar * abs(ref)
    for li, d in enumerate(grads):
        for c, got in zip("qkv", QM.unpack(d, 2)):
            want = torch.from_numpy(g[f"{name}{npairs}_grad_{li}{c}"]).to(F64)
            assert float((got - want).abs().max()) <= bar * float(want.abs().max()), (li, c)


def test_soft_cross_entropy_vs_golden(golden):
    """soft_cross_entropy itself: float64 against the reference's fp32 run, to 2^-23 (C + 16) max|x| as above (C <= 7)"""
    g = golden("qkvce")
    for i, (p, t) in enumerate(QM.golden_ce_inputs()):
        loss, dp, _, _ = QM.soft_ce_bounds(p, t)
        bar = 2.0 ** -23 * (7 + 16) * float(max(p.abs().max(), t.abs().max()))
        assert abs(float(loss) - float(g[f"ce{i}_loss"])) <= bar * abs(float(loss))
        want = torch.from_numpy(g[f"ce{i}_grad"]).to(F64)
        assert float((dp - want).abs().max()) <= bar * float(want.abs().max())


@pytest.mark.parametrize("layout", ["view", "tokens"])
@pytest.mark.parametrize("cross", [False, True])
@pytest.mark.parametrize("B,N,Ds,Dt", [(2, 5, 128, 192), (1, 17, 384, 768)])
def test_restatement_vs_autograd(B, N, Ds, Dt, cross, layout):
    """the analytic backward against torch autograd of the definition, both in float64: 1e-13 of the scale of the terms that cancel in it (S is c times
    four probabilities <= 1, times |X|: near one-hot rows of student and teacher leave a gradient far below that scale); the loss to 1e-13
    absolute (its terms are differences lse - z of numbers of size |Z| <= 30: near one-hot rows leave a loss of 1e-4 from terms that large)"""
    xs, xt, up = QM.inputs(B, N, Ds, Dt, "sharp")
    x = xs.clone().requires_grad_(True)
    loss = QM.definition(x, xt, cross, layout, layers=2)
    (loss * up).backward()
    r = QM.restate(xs, xt, cross, layout, layers=2, upstream=up)
    assert abs(float(r["loss"]) - float(loss.detach())) <= 1e-13
    assert float((r["d"] - x.grad).abs().max()) <= 1e-13 * 4 * abs(r["c"]) * float(xs.abs().max())


def test_view_layout_is_the_reference_s_view():
    """rows(..., "view") gathers exactly what `.contiguous().view(B, N, H * 64)` of [B, H, N, 64] reinterprets, and the definition on packed buffers is
    the reference's form on the tuples"""
    stu, tea = QM.golden_inputs()
    for qkv in stu + tea:
        B, H, N, C = qkv[0].shape
        x = QM.pack(qkv)
        for i in range(3):
            assert torch.equal(QM.rows(x, i, "view"), qkv[i].contiguous().view(B, N, H * C))
            assert torch.equal(QM.rows(x, i, "tokens"), qkv[i].permute(0, 2, 1, 3).reshape(B, N, H * C))
    for cross in (False, True):
        a = QM.reference_form([tuple(x.to(F64) for x in q) for q in stu], [tuple(x.to(F64) for x in q) for q in tea], cross)
        b, _ = QM.cal(stu, tea, cross, "view")
        assert abs(float(a) - float(b)) <= 1e-14 * float(a)


@pytest.mark.parametrize("H", [2, 3, 6, 12])
@pytest.mark.parametrize("N", [5, 17, 197, 198])
def test_view_map_is_a_bijection(N, H):
    """every (head, token) chunk of an image is chunk m of exactly one row r; rows straddle heads whenever N % H != 0"""
    h, n = QM.chunk_map(N, H, "view")
    assert int(h.min()) == 0 and int(h.max()) == H - 1 and int(n.min()) == 0 and int(n.max()) == N - 1
    assert len(set((h * N + n).flatten().tolist())) == N * H
    straddles = bool((h.min(1).values != h.max(1).values).any())
    assert straddles == (N % H != 0)
    ht, nt = QM.chunk_map(N, H, "tokens")
    assert torch.equal(ht[0], torch.arange(H)) and torch.equal(nt[:, 0], torch.arange(N))
    if H == 1:
        assert torch.equal(h, ht) and torch.equal(n, nt)


@pytest.mark.parametrize("regime", QM.REGIMES)
@pytest.mark.parametrize("B,N,Ds,Dt", QM.CASES)
def test_emulation_inside_bounds(B, N, Ds, Dt, regime):
    """fp32 arithmetic with ONE bf16 rounding of S and of d stays inside the per-element bounds at every shape and regime of the GPU test (the cross
    mode: its nine slots hold the self mode's three)"""
    xs, xt, up = _case(B, N, Ds, Dt, regime)
    r, bnd = QM.bounds(xs, xt, True, "view", layers=1, upstream=up)
    e = QM.emulate(xs, xt, True, "view", layers=1, upstream=up)
    worst = dict(loss=QM.ratio(e["loss"].to(F64), r["loss"], bnd["loss"]), d=QM.ratio(e["d"], r["d"], bnd["d"]))
    assert all(v <= 1.0 for v in worst.values()), worst
    if regime == "same":
        assert float(r["d"].abs().max()) == 0.0


@pytest.mark.parametrize("cross", [False, True])
@pytest.mark.parametrize("layout", ["view", "tokens"])
def test_emulation_inside_bounds_modes(cross, layout):
    for regime in ("sharp", "flat"):
        xs, xt, up = _case(2, 17, 128, 256, regime)
        r, bnd = QM.bounds(xs, xt, cross, layout, layers=2, upstream=up)
        e = QM.emulate(xs, xt, cross, layout, layers=2, upstream=up)
        assert QM.ratio(e["loss"].to(F64), r["loss"], bnd["loss"]) <= 1.0 and QM.ratio(e["d"], r["d"], bnd["d"]) <= 1.0


@pytest.mark.parametrize("mutate", QM.MUTATIONS)
def test_bounds_can_fail(mutate):
    """each of four wrong kernels leaves the bounds in at least one regime: the model is not wide enough to hide them"""
    left = {}
    for regime in ("sharp", "flat"):
        xs, xt, up = _case(2, 17, 128, 256, regime)
        for cross in (False, True):
            r, bnd = QM.bounds(xs, xt, cross, "view", upstream=up)
            e = QM.emulate(xs, xt, cross, "view", upstream=up, mutate=mutate)
            left[(regime, cross)] = max(QM.ratio(e["loss"].to(F64), r["loss"], bnd["loss"]), QM.ratio(e["d"], r["d"], bnd["d"]))
    assert max(left.values()) > 1.0, left


def test_list_form_divides_by_the_number_of_pairs():
    stu, tea = QM.golden_inputs()
    for cross in (False, True):
        both, gb = QM.cal(stu, tea, cross)
        one = [QM.cal([s], [t], cross) for s, t in zip(stu, tea)]
        assert abs(float(both) - float(sum(o[0] for o in one)) / 2) <= 1e-15
        assert float((gb[0] - one[0][1][0] / 2).abs().max()) <= 1e-18


def test_cli_qkv_flags():
    """--qkv-ce-gama / --qkv-cross-gama: default 0, any value >= 0 accepted, a negative one refused by the parser; --qkv-layout view | tokens"""
    import distill_sub
    p = distill_sub.get_args_parser()
    a = p.parse_args([])
    assert (a.qkv_ce_gama, a.qkv_cross_gama, a.qkv_layout) == (0.0, 0.0, "view")
    a = p.parse_args(["--qkv-ce-gama", "0.3", "--qkv-cross-gama", "0.1", "--qkv-layout", "tokens"])
    assert a.qkv_ce_gama == pytest.approx(0.3) and a.qkv_cross_gama == pytest.approx(0.1) and a.qkv_layout == "tokens"
    for flag in ("--qkv-ce-gama", "--qkv-cross-gama"):
        for bad in ("-0.1", "nan"):
            with pytest.raises(SystemExit):
                p.parse_args([flag, bad])
    with pytest.raises(SystemExit):
        p.parse_args(["--qkv-layout", "heads"])


def test_engine_refuses_negative_weights():
    from devit_amd import engine
    for kw in (dict(qkv_ce_gama=-1.0), dict(qkv_cross_gama=-0.5), dict(qkv_ce_gama=float("nan")), dict(qkv_layout="heads")):
        with pytest.raises(ValueError):
            engine.distill_forward(torch.nn.Identity(), torch.nn.Identity(), None, None, **kw)


def test_losses_refuse_cpu_tensors():
    import devit_amd
    from devit_amd._lib import DevitError
    q = torch.zeros(1, 2, 5, 64)
    for fn in (devit_amd.cal_qkv_loss, devit_amd.cal_qkv_loss2):
        with pytest.raises(DevitError):
            fn([(q, q, q)], [(q, q, q)])
    with pytest.raises(DevitError):
        devit_amd.soft_cross_entropy(torch.zeros(3, 7), torch.zeros(3, 7))
