"""tests/_gemm_model.py under test, without a GPU: every emulation stays inside its bound, every planted bug leaves it, every case of the table
reaches the kernel instantiation it names -- asked of devit_gemm_route, the selection rule itself -- and the table covers exactly the instantiations
that exist; the fitted GELU's documented accuracy and its clamp hold on a dense grid.  tests/test_gpu_gemm.py runs the same table on the kernels."""
import math

import pytest
import torch

import _gemm_model as G
from _gemm_model import ATOMIC, DGELU, F64, FULL_ROW, GELU, GEMM4, PATCH, RESIDUAL, STORE_BF16, STORE_F32, TILE128, TILE256

CASES = G.cases()
FWD = (STORE_BF16, GELU, RESIDUAL, PATCH, STORE_F32)

# Every (route, layout variant = 2 (A k-major) + (B k-major), epilogue kind, dtype16) that is instantiated: launch_gemm_tile's switch
# (gemm_tile.h: the forward layouts in both 16-bit types through launch_fwd, k-major B in bf16, k-major x k-major on 128x128 tiles only),
# launch_gemm4's switch (gemm4.hip) and launch_gemmfr (gemmfr.hip; its LayerNorm-backward variant belongs to test_gpu_lnfuse.py).  35.
INSTANTIATED = (
    [(t, 0, k, d) for t in (TILE128, TILE256) for k in FWD for d in (0, 1)] +
    [(t, 1, k, 0) for t in (TILE128, TILE256) for k in (STORE_BF16, STORE_F32, DGELU)] +
    [(TILE128, 3, ATOMIC, 0), (TILE128, 3, STORE_F32, 0)] +
    [(GEMM4, 0, k, 0) for k in FWD] +
    [(FULL_ROW, 1, STORE_BF16, 0), (FULL_ROW, 1, RESIDUAL, 0)])

# fp32 outputs held below 1 instead of at 0.5, by name, as _tail_model.SHORT_PATHS: at K = 64 the accumulator term of the bound (E32 K sum|a||b|) is
# small, and where a bias of magnitude up to 30 (or the residual) stands beside a 2^-6 row of A the
# output is ONE rounding of a value of its own magnitude -- acc + bias (gemm_device.h:300), + pos / the residual sum (:315-316).  The bound is then
# the worst case of a correct implementation, which some element of a hundred thousand comes close to.  Every other fp32 output stays at <= 0.5.
SHORT_F32 = {"t128/store_f32/K64/bf16": "acc + bias: 1", "t128/kmB/store_f32/K64": "acc + bias: 1",
             "t128/patch_tok1/K64/bf16": "acc + bias, + pos: 2", "t128/patch_tok1/K64/f16": "acc + bias, + pos: 2",
             "t128/residual_alias/K64/bf16": "acc + bias, rowscale *, res +: 3",
             "t128/gram_batch3/K64": "acc + bias: 1 (the operands are scaled by 1/8: a bias of magnitude 8 beside sum|a||b| = 8e-4 at the worst element)"}


def route_of(c, inp):
    from devit_amd import ops
    args, kw = G.call_args(c, inp, G.fake_address)
    return ops.gemm_route(*args, **kw)


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_case_reaches_its_route_and_its_emulation_holds(c, monkeypatch):
    inp = G.inputs(c)
    G.set_route_env(monkeypatch, c)
    assert route_of(c, inp) == c["route"], f"{c['name']}: the selection rule sends this shape to another kernel than the table says"
    rt, untouched = G.verdict(c, inp, G.emulate(c, inp))
    assert untouched
    for name, r in rt.items():
        one = name == "aux" and c["kind"] != ATOMIC or c["kind"] in G.OUT16 or c["name"] in SHORT_F32
        assert r < 1.0 if one else r <= 0.5, (c["name"], name, r)


def test_table_covers_every_instantiation():
    got = {G.instantiation(c) for c in CASES}
    assert len(INSTANTIATED) == len(set(INSTANTIATED)) == 35
    assert got == set(INSTANTIATED), (sorted(got - set(INSTANTIATED)), sorted(set(INSTANTIATED) - got))
    for route in (TILE128, TILE256, GEMM4, FULL_ROW):
        assert any(c["integer"] and c["route"] == route for c in CASES), "one exact-integer variant per route"
        assert any(c["reserve"] and c["route"] == route for c in CASES), "one more-than-one-tile-per-workgroup case per persistent kernel"


def test_route_reports_refusals_without_a_device(monkeypatch):
    """devit_gemm_route returns the DEVIT_ERR_* of devit_gemm_bf16's argument checks (the launches themselves: tests/test_gpu_gemm.py)"""
    c = G.case_named("t128/store_f32/K192/bf16")
    inp = G.inputs(c)
    G.set_route_env(monkeypatch, c)
    assert route_of(dict(c, M=192), inp) == -1
    assert route_of(dict(c, K=96), inp) == -1
    assert route_of(dict(c, split_k=2), inp) == -2
    # the full-row kernel is what DEVIT_GEMMFR says, read per call
    f = G.case_named("fr/store_bf16/K192")
    finp = G.inputs(f)
    monkeypatch.setenv("DEVIT_GEMMFR", "1")
    assert route_of(f, finp) == FULL_ROW
    monkeypatch.setenv("DEVIT_GEMMFR", "0")
    assert route_of(f, finp) == TILE128
    r = G.case_named("fr/residual/K256")
    assert route_of(r, G.inputs(r)) == -2, "a k-major residual off the full-row kernel is refused"


# ---- planted bugs: (mutation, case, output) -- the output's ratio must reach 1 (inf: non-finite values or an exact-integer mismatch), or, for
# output None, a sentinel must change
PLANTED = [("last_product_dropped", "t128/store_f32/K192/bf16", "out"), ("last_product_dropped", "t256/store_f32/K384/int", "out"),
           ("last_product_dropped", "fr/store_bf16/K192", "out"),
           ("bias_from_left_at_tile_edge", "t128/store_f32/K192/bf16", "out"), ("bias_from_left_at_tile_edge", "g4/store_f32/K384", "out"),
           ("colscale_on_saved_preactivation", "t128/gelu/K192/bf16", "aux"), ("colscale_on_saved_preactivation", "t256/gelu/K64/f16", "aux"),
           ("rowscale_tile_local", "t256/residual/K1536/bf16", "out"), ("rowscale_tile_local", "fr/residual/K256", "out"),
           ("m_valid_plus_one", "t128/store_bf16/K192/bf16", None), ("m_valid_plus_one", "t128/kmAB/atomic_split1_aux/K192", None),
           ("row_skip_without_plus_one", "t128/kmAB/atomic_patch_wgrad/K3136", "out"),
           ("row_skip_without_plus_one", "t128/kmB/store_bf16_rowgroup/K192", "out"),
           ("patch_without_tok", "t128/patch_tok2/K192/bf16", "out"), ("patch_without_tok", "t128/patch_tok1/K64/f16", "out"),
           ("gelu_without_clamp", "t128/gelu/K192/bf16", "out"), ("gelu_without_clamp", "t256/gelu/K192/f16", "out"),
           ("f16_store_through_bf16", "t128/store_bf16/K192/f16", "out"), ("f16_store_through_bf16", "t128/gelu/K192/f16", "aux"),
           ("split_slice_twice", "t128/kmAB/atomic_split3/K192", "out"), ("split_slice_twice", "t128/kmAB/atomic_split2/K192/int", "out")]


@pytest.mark.parametrize("mutate,case,output", PLANTED)
def test_planted_bug_is_seen(mutate, case, output):
    c = G.case_named(case)
    inp = G.inputs(c)
    rt, untouched = G.verdict(c, inp, G.emulate(c, inp, mutate=mutate))
    if output is None:
        assert not untouched, (mutate, case)
    else:
        assert rt[output] >= 1.0, (mutate, case, output, rt[output])


def test_every_mutation_is_planted_somewhere():
    assert {m for m, _, _ in PLANTED} | {"colsum_of_wrong_operand"} == set(G.MUTATIONS)


# ---- devit_wgrad_grouped
@pytest.mark.parametrize("name,K,split,jobs", G.wgrad_cases(), ids=[w[0] for w in G.wgrad_cases()])
def test_wgrad_emulation_holds(name, K, split, jobs):
    s = split or G.wgrad_max_split(K)
    for d in G.wgrad_inputs(name, K, jobs)[:6]:
        rt, untouched = G.wgrad_verdict(d, G.wgrad_emulate(d, K, s), G.wgrad_reference(d, K, s))
        assert untouched and all(r <= 0.5 for r in rt.values()), (name, d["job"]["name"], rt)


@pytest.mark.parametrize("case,job", [("K192_split1", "wide_t"), ("K192_int", "int_t"), ("K192_split1", "half")])
def test_wgrad_planted_bug_is_seen(case, job):
    """a_colsum taken over the wrong operand -- on the TRANSPOSED jobs (a_cols 1152 and the integer one), where the roles of a and b swap in `out`
    while the sum must stay over a; and on a plain job"""
    name, K, split, jobs = next(w for w in G.wgrad_cases() if w[0] == case)
    d = next(x for x in G.wgrad_inputs(name, K, jobs) if x["job"]["name"] == job)
    assert d["job"]["colsum"] and d["job"]["transposed"] == (job != "half")
    rt, _ = G.wgrad_verdict(d, G.wgrad_emulate(d, K, split, mutate="colsum_of_wrong_operand"), G.wgrad_reference(d, K, split))
    assert rt["colsum"] >= 1.0 and rt["out"] <= 0.5, rt


# ---- the fitted GELU's documented accuracy (devit_common.h:78, repeated in gemm.hip's exact_gelu refusal) and its clamp
def test_fitted_gelu_meets_its_documented_accuracy():
    """float64 restatement of gelu_fwd<false> / gelu_bwd<false> with the three fp32 constants (read from the header text) against the erf form on
    2,000,001 points of [-40, 40].  The constants come from devit_common.h: tools/fit_gelu.py refits them with scipy and exposes none."""
    x = torch.linspace(-40, 40, 2_000_001, dtype=F64)
    e_f = (G.gelu_fit(x) - G.gelu_exact(x)).abs()
    e_b = (G.dgelu_fit(x) - G.dgelu_exact(x)).abs()
    i, j = int(e_f.argmax()), int(e_b.argmax())
    print(f"gelu fit: {float(e_f[i]):.4e} at x = {float(x[i]):+.3f}; gelu' fit: {float(e_b[j]):.4e} at x = {float(x[j]):+.3f}")
    assert (G.GELU_FIT_ERR, G.DGELU_FIT_ERR) == (2.6e-5, 1.2e-4), "the documented figures the bounds of _gemm_model add"
    assert float(e_f[i]) <= G.GELU_FIT_ERR and float(e_b[j]) <= G.DGELU_FIT_ERR
    assert abs(abs(float(x[i])) - 0.566) < 2e-3 and abs(abs(float(x[j])) - 0.934) < 2e-3     # where the fit is worst: inside [-8, 8]
    # the clamp: x^2 <= 36 is what keeps the polynomial from turning over -- without it the fitted form leaves the erf form by more than 1 from
    # |x| = 11.2 on (c0 + c1 x^2 + c2 x^4 changes sign at x^2 = 123.4), with it the two figures hold out to |x| = 40
    assert G.GELU_CLAMP == 36.0
    far = x.abs() >= 6
    assert float(e_f[far].max()) <= G.GELU_FIT_ERR and float(e_b[far].max()) <= G.DGELU_FIT_ERR
    assert float((G.gelu_fit(x, clamp=False) - G.gelu_exact(x)).abs()[x.abs() >= 11.2].max()) > 1.0
    # the fp32 emulation's GELU is that function: within the arithmetic term of the bound (_fit_arith) on [-12, 12]
    x = torch.linspace(-12, 12, 100_001, dtype=F64).float()
    e_s = G._fit_arith(x.double())[0]
    assert bool(((G.gelu_fit32(x).double() - G.gelu_fit(x.double())).abs() <= x.double().abs() * e_s + 2 * G.U * x.double().abs()).all())


def test_ratio_semantics():
    one = torch.ones(3, dtype=F64)
    assert G.ratio(one, one, 0 * one) == 0.0 and G.ratio(one + 1, one, 0 * one) == math.inf
    assert G.ratio(torch.tensor([1.0, math.nan]), torch.ones(2), torch.ones(2)) == math.inf
