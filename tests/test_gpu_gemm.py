"""The 16-bit MFMA GEMM family -- devit_gemm_bf16 on its four kernels (gemm_kernel on 128x128 and 256x256 tiles, gemm4_kernel, gemmfr_kernel) and
devit_wgrad_grouped -- on a real MI355X against the float64 statements of tests/_gemm_model.py, on the case table and the inputs
tests/test_gemm_model.py holds the model itself to.  Each case
    asks devit_gemm_route (the selection rule itself) that the launch reaches the kernel instantiation the table names,
    launches through ops.gemm,
    holds EVERY live output element below its first-order bound: chk(worst |err| / bound, 1.0, name="gemm/<case>/<output>"), torch.equal in the
    exact-integer variants,
    and checks that the call wrote nothing else: rows >= m_valid, the pad columns of ldc = N + 8, the gaps between batches, the token rows of a PATCH
    output and the guards behind every buffer come back bit for bit.
Everything of an input buffer that the operand description does not name holds NaN (pad columns inside lda / ldb, the rows row_skip steps over, res
and aux_in rows >= m_valid, bias / colscale / rowscale / pos past their extent, pos rows below extra_tokens): a kernel that reads it stores a
non-finite value, which ratio() reports as inf.  Rows of a row-major A at or above m_valid are read and never stored: finite junk and one inf.
The float64 reference is computed with torch on the device.  Every refusal below is the entry point's argument check: nothing is launched."""

import pytest
import torch

import _gemm_model as G
from conftest import chk

pytestmark = pytest.mark.gpu

CASES = G.cases()
WCASES = G.wgrad_cases()


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from devit_amd import _lib
    _lib.require_device(torch.zeros(1, device="cuda"))
    return torch.device("cuda")


def hold(tag, r):
    print(f"gemm/{tag} {r:.4f}")
    assert chk(r, 1.0, name=f"gemm/{tag}"), f"gemm/{tag}: worst |err| / bound {r:.4f}"


def buffers(inp):
    """the buffers the call writes (fresh copies of the preloaded ones) and at(): the tensor view that stands for a named buffer from an element on"""
    got = {"out": inp["bufs"]["out0"].clone()}
    if "aux0" in inp["bufs"]:
        got["aux"] = inp["bufs"]["aux0"].clone()

    def at(name, off):
        return (got[name] if name in got else inp["bufs"][name])[off:]
    return got, at


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_gemm_case(dev, c, monkeypatch):
    from devit_amd import _lib as L, ops
    G.set_route_env(monkeypatch, c)
    lib = L.load()
    before = lib.devit_get_reserved_cus()
    if c["reserve"]:
        # more than one tile per workgroup at small size.  The premise restates two lines of gemm.hip and must move with them: persistent_grid()
        # (gemm.hip:34-37: (CUs - reserved, at least 8) x occupancy, rounded down to a multiple of 8) and gemm_launch's `bm`, `bn`, `occ`
        # (G.tiles_of).  If either changes, this computation is what to update: a grid that grew past the tile count would leave the case
        # passing on one tile per workgroup.
        cus = torch.cuda.get_device_properties(dev).multi_processor_count
        left = (cus - c["reserve"]) * G.tiles_of(c)[2] // 8 * 8
        if cus - c["reserve"] < 8 or G.tile_count(c) <= left:
            pytest.skip(f"{cus} CUs: with {c['reserve']} reserved the grid of {left} workgroups still gives each of the {G.tile_count(c)} tiles its own")
    inp = G.to_device(G.inputs(c), dev)
    got, at = buffers(inp)
    args, kw = G.call_args(c, inp, at)
    assert ops.gemm_route(*args, **kw) == c["route"], f"{c['name']}: the selection rule sends this shape to another kernel than the table says"
    try:
        if c["reserve"]:
            L.call("devit_set_reserved_cus", c["reserve"])
        ops.gemm(*args, **kw)
        torch.cuda.synchronize()
    finally:
        if c["reserve"]:
            L.call("devit_set_reserved_cus", before)
    rt, untouched = G.verdict(c, inp, got)
    assert untouched, f"{c['name']}: a write outside what the call describes (rows >= m_valid, pad columns, token rows, gaps or guards changed)"
    for name, r in rt.items():
        hold(f"{c['name']}/{name}", r)


@pytest.mark.parametrize("name,K,split,jobs", WCASES, ids=[w[0] for w in WCASES])
def test_wgrad_grouped(dev, name, K, split, jobs):
    """devit_wgrad_grouped -- the entry point ops.linear_wgrads calls, here with leading dimensions wider than the matrices, which that wrapper
    cannot express.  split_k == 0: the bound counts the most slices the cost model can choose (wgradfr.hip:267)."""
    from devit_amd import _lib as L, ops
    ds = [{k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in d.items()} for d in G.wgrad_inputs(name, K, jobs)]
    gots, structs = [], []
    for d in ds:
        got = {"out": d["out0"].clone()}
        if "colsum0" in d:
            got["colsum"] = d["colsum0"].clone()
        j = L.WgradJob(d["a"].data_ptr(), d["lda"], d["job"]["a_cols"], d["b"].data_ptr(), d["ldb"], got["out"].data_ptr(), d["ldc"],
                       d["job"]["transposed"], got["colsum"].data_ptr() if "colsum" in got else None)
        gots.append(got)
        structs.append(j)
    ops.call("devit_wgrad_grouped", (L.WgradJob * len(structs))(*structs), len(structs), K, split, L.stream_ptr())
    torch.cuda.synchronize()
    s = split or G.wgrad_max_split(K)
    worst = {}
    for d, got in zip(ds, gots):
        rt, untouched = G.wgrad_verdict(d, got, G.wgrad_reference(d, K, s))
        assert untouched, f"wgrad/{name}/{d['job']['name']}: a write outside the accumulator"
        for k, r in rt.items():
            key = f"wgrad_{name}/{d['job']['name'] if len(ds) <= 8 else 'jobs'}/{k}"
            worst[key] = max(worst.get(key, 0.0), r)
    for key, r in worst.items():
        hold(key, r)


# ---- refusals: calls the header forbids return their exact DEVIT_ERR_* and write nothing
ARG_NAMES = ("a", "lda", "a_km", "b", "ldb", "b_km", "M", "N", "K")
REFUSALS = [
    ("M_not_a_multiple_of_128", "t128/store_f32/K192/bf16", dict(M=192), {}, -1, "must be multiples"),
    ("K_not_a_multiple_of_64", "t128/store_f32/K192/bf16", dict(K=96), {}, -1, "must be multiples"),
    ("split_k_without_atomic", "t128/store_f32/K192/bf16", dict(split_k=2), {}, -2, "split_k"),
    ("f16_with_a_kmajor_operand", "t128/store_f32/K192/f16", dict(b_km=1, ldb=392), {}, -2, "f16 operands"),
    ("f16_dgelu", "t128/kmB/dgelu/K192", dict(dtype16=1, b_km=0, ldb=200), {}, -2, "f16 operands"),
    ("dgelu_with_a_bias", "t128/kmB/dgelu/K192", dict(bias="colscale"), {}, -2, "takes no bias"),
    ("row_group_on_a_row_major_operand", "t128/store_f32/K192/bf16", dict(a_group=48, a_skip=3), {}, -2, "row_group/skip only"),
    ("kmajor_residual_off_the_full_row_kernel", "fr/residual/K256", {}, {"DEVIT_GEMMFR": "0"}, -2, "full-row kernel only"),
    ("exact_gelu", "t128/gelu/K192/bf16", dict(exact_gelu=1), {}, -2, "exact_gelu=1"),
    ("misaligned_ldc", "t128/store_f32/K192/bf16", dict(ldc=388), {}, -2, "16-byte aligned"),
]


@pytest.mark.parametrize("tag,case,change,env,rc,text", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_gemm_refuses(dev, monkeypatch, tag, case, change, env, rc, text):
    from devit_amd import _lib as L, ops
    c = G.case_named(case)
    G.set_route_env(monkeypatch, dict(c, env=dict(c["env"], **env)))
    inp = G.to_device(G.inputs(c), dev)
    got, at = buffers(inp)
    args, kw = G.call_args(c, inp, at)
    args = list(args)
    for k, v in change.items():
        v = at(v, 0) if isinstance(v, str) else v
        if k in ARG_NAMES:
            args[ARG_NAMES.index(k)] = v
        else:
            kw[k] = v
    assert ops.gemm_route(*args, **kw) == rc
    with pytest.raises(L.DevitError, match=rf"devit_gemm_bf16 failed \({rc}\)") as e:
        ops.gemm(*args, **kw)
    assert text in str(e.value), str(e.value)
    torch.cuda.synchronize()
    for name, t in got.items():
        assert torch.equal(t.view(torch.int16), inp["bufs"][name + "0"].view(torch.int16)), f"{tag}: a refused call wrote to {name}"


@pytest.mark.parametrize("tag,K,split,njobs,rc,text", [("fewer_than_3_ksteps_per_slice", 192, 2, 1, -1, "fewer than 3"), ("49_jobs", 192, 1, 49, -2, "jobs")])
def test_wgrad_grouped_refuses(dev, tag, K, split, njobs, rc, text):
    from devit_amd import _lib as L, ops
    d = {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in G.wgrad_inputs("refuse", K, [G._wjob("half", 128)])[0].items()}
    out, cs = d["out0"].clone(), d["colsum0"].clone()
    j = L.WgradJob(d["a"].data_ptr(), d["lda"], 128, d["b"].data_ptr(), d["ldb"], out.data_ptr(), d["ldc"], 0, cs.data_ptr())
    with pytest.raises(L.DevitError, match=rf"devit_wgrad_grouped failed \({rc}\)") as e:
        ops.call("devit_wgrad_grouped", (L.WgradJob * njobs)(*([j] * njobs)), njobs, K, split, L.stream_ptr())
    assert text in str(e.value), str(e.value)
    torch.cuda.synchronize()
    assert torch.equal(out, d["out0"]) and torch.equal(cs, d["colsum0"]), f"{tag}: a refused call wrote"
