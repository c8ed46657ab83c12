"""The student's dgrad + LayerNorm backward as ONE launch of the full-row GEMM (csrc/gemmfr.hip, epilogue kind LNBWD; devit_dgrad_layernorm_bwd):
the fused launch against the two launches it replaces, on the same inputs, at the step's shapes.

dx and dx_bf16 must be the SAME BITS: the epilogue stages the tile's rows in LDS and runs ln_bwd_kernel's own row body on them (csrc/ln_rows.h).
dgamma / dbeta / the column sums of dx_bf16 add the same fp32 terms in another order; their bound is derived from the inputs:
    |a - b| <= eps_fp32 * (longest chain of additions a term goes through, either path) * sum |terms|   (the sum in fp64),
i.e. each path is within unit-roundoff * chain * sum |terms| of the exact sum (Higham, Accuracy and Stability, section 4.2) and eps = 2 units."""
import pytest
import torch

pytestmark = pytest.mark.gpu
BF16, F32 = torch.bfloat16, torch.float32
N, D = 198, 384
SENTINEL = 7.0


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda")


def make_inputs(dev, B, K, seed):
    """One site's operands: dy [Mp][K] bf16 (pad rows hold finite junk AND an inf: nothing of them may reach a live row), the weight [K][D],
    the forward input x with its saved statistics, the upstream residual gradient, a per-image scale."""
    from devit_amd import ops
    M = B * N
    g = torch.Generator(device=dev).manual_seed(seed)
    dy = ops.rows_alloc(M, K, BF16, dev)
    dy[:M] = (torch.randn((M, K), generator=g, device=dev) * 0.5).to(BF16)
    if dy.shape[0] > M:
        dy[M:] = (torch.randn((dy.shape[0] - M, K), generator=g, device=dev) * 40).to(BF16)
        dy[M, ::7] = float("inf")
    w = (torch.randn((K, D), generator=g, device=dev) * 0.05).to(BF16)
    x = torch.randn((M, D), generator=g, device=dev) * 2.0 + 0.3
    gm = 1 + 0.1 * torch.randn(D, generator=g, device=dev)
    mean, rstd = torch.empty(M, device=dev), torch.empty(M, device=dev)
    ops.layernorm_fwd(x, M, D, gm, torch.zeros(D, device=dev), 1e-6, y_bf16=torch.empty((M, D), dtype=BF16, device=dev), mean=mean, rstd=rstd)
    dres = torch.randn((M, D), generator=g, device=dev)
    rsc = (torch.arange(B, device=dev) % 7 != 0).float() / 0.9
    return dict(M=M, Mp=dy.shape[0], K=K, dy=dy, w=w, x=x, gm=gm, mean=mean, rstd=rstd, dres=dres, rsc=rsc)


def launch(inp, *, rowscale=True, dres=True, bf16=True):
    """devit_dgrad_layernorm_bwd on `inp`; whatever path the library's rule picks.  Outputs carry SENTINEL rows past M and a SENTINEL dln:
    the fused launch never writes dln, the unfused one does -- that is how the tests know which one ran."""
    from devit_amd import ops, _lib as L
    from devit_amd._lib import call, ptr, stream_ptr
    dev, M, Mp, K = inp["x"].device, inp["M"], inp["Mp"], inp["K"]
    dln = torch.full((Mp, D), SENTINEL, dtype=BF16, device=dev)
    dx = torch.full((Mp, D), SENTINEL, dtype=F32, device=dev)
    dxb = torch.full((Mp, D), SENTINEL, dtype=BF16, device=dev) if bf16 else None
    dg, db = torch.zeros(D, device=dev), torch.zeros(D, device=dev)
    gs = torch.zeros(D, device=dev) if bf16 else None
    ws = ops.workspace(dev, L.load().devit_layernorm_bwd_workspace(M, D))
    call("devit_dgrad_layernorm_bwd", ptr(inp["dy"]), ptr(inp["w"]), Mp, K, ptr(dln), ptr(inp["x"]), M, D, ptr(inp["mean"]), ptr(inp["rstd"]),
         ptr(inp["gm"]), ptr(inp["dres"] if dres else None), ptr(dx), ptr(dxb), ptr(inp["rsc"] if rowscale else None), N, ptr(dg), ptr(db), ptr(gs), 1,
         ptr(ws), ws.numel(), stream_ptr())
    torch.cuda.synchronize()
    return dict(dln=dln, dx=dx, dxb=dxb, dg=dg, db=db, gs=gs, wrote_dln=bool((dln[:M] != SENTINEL).any()))


def pads_untouched(inp, out):
    M = inp["M"]
    return bool((out["dx"][M:] == SENTINEL).all()) and (out["dxb"] is None or bool((out["dxb"][M:] == SENTINEL).all()))


def chain_length(M):
    """Longest chain of fp32 additions a term goes through on its way into dgamma / dbeta / the column sums: rows of one half-wave, the two
    half-waves, the four waves, colsum_partials_kernel's strided pass over the partials and its 32-way finish, the accumulate into the output."""
    tiles = (M + 255) // 256
    grid = min(1024, (M + 7) // 8)
    unfused = -(-M // (grid * 8)) + 1 + 3 + -(-grid // 32) + 32 + 1
    fused = 32 + 1 + 3 + -(-tiles // 32) + 32 + 1
    return max(unfused, fused)


def check_column_sums(inp, ref, got):
    """ref = the unfused launches (its dln holds the bf16 dy both paths fed the LayerNorm with)."""
    M = inp["M"]
    eps = torch.finfo(F32).eps
    dy = ref["dln"][:M].float()
    xh = (inp["x"] - inp["mean"][:, None]) * inp["rstd"][:, None]          # fp32, the kernels' own two operations
    bound_g = eps * chain_length(M) * (dy.double() * xh.double()).abs().sum(0)
    bound_b = eps * chain_length(M) * dy.double().abs().sum(0)
    for name, bound in (("dg", bound_g), ("db", bound_b)):
        err = (ref[name].double() - got[name].double()).abs()
        print(f"{name}: max |diff| {float(err.max()):.3e}, smallest bound {float(bound.min()):.3e}, worst diff / bound {float((err / bound).max()):.3e}")
        assert bool((err <= bound).all()), name
    if ref["gs"] is not None:
        bound = eps * chain_length(M) * ref["dxb"][:M].double().abs().sum(0)
        err = (ref["gs"].double() - got["gs"].double()).abs()
        print(f"gs: max |diff| {float(err.max()):.3e}, smallest bound {float(bound.min()):.3e}, worst diff / bound {float((err / bound).max()):.3e}")
        assert bool((err <= bound).all()), "gs"


FLAGS = {"all": dict(rowscale=True, dres=True, bf16=True), "none": dict(rowscale=False, dres=False, bf16=False),
         "bf16_unscaled": dict(rowscale=False, dres=True, bf16=True), "no_dres": dict(rowscale=True, dres=False, bf16=True)}


@pytest.mark.parametrize("B,K,flags", [
    (256, 1536, "all"), (256, 1536, "none"), (256, 1536, "bf16_unscaled"), (256, 1536, "no_dres"),      # fc1's dgrad + LN2 backward
    (256, 1152, "all"), (256, 1152, "none"),                                                              # qkv's dgrad + LN1 backward (g_prev NULL in block 0)
    (256, 768, "all"),                                                                                    # the compacted student's qkv (4 of 6 heads)
    (250, 1536, "all"), (250, 1152, "none")])                                                             # ragged: 49500 rows = 194 tiles, the last with 92 rows
def test_fused_matches_unfused(dev, monkeypatch, B, K, flags):
    from devit_amd import _lib as L
    inp = make_inputs(dev, B, K, 100 + K + B)
    monkeypatch.setenv("DEVIT_LNFUSE", "0")
    assert L.load().devit_dgrad_layernorm_bwd_fused(inp["Mp"], D, K) == 0
    ref = launch(inp, **FLAGS[flags])
    assert ref["wrote_dln"]
    monkeypatch.setenv("DEVIT_LNFUSE", "1")
    assert L.load().devit_dgrad_layernorm_bwd_fused(inp["Mp"], D, K) == 1
    got = launch(inp, **FLAGS[flags])
    assert not got["wrote_dln"], "the fused launch was expected (it does not write dln)"
    assert pads_untouched(inp, ref) and pads_untouched(inp, got)
    M = inp["M"]
    assert bool(torch.isfinite(got["dx"][:M]).all())
    assert torch.equal(ref["dx"], got["dx"])
    if ref["dxb"] is not None:
        assert torch.equal(ref["dxb"], got["dxb"])
    check_column_sums(inp, ref, got)


def test_fused_launch_is_reproducible(dev, monkeypatch):
    """Twenty launches on the same inputs: the same bits every time, column sums included (no atomics; a missing barrier between the staging
    writes and the row reads would show here)."""
    monkeypatch.setenv("DEVIT_LNFUSE", "1")
    inp = make_inputs(dev, 250, 1536, 7)
    first = launch(inp)
    assert not first["wrote_dln"]
    for i in range(19):
        again = launch(inp)
        for k in ("dx", "dxb", "dg", "db", "gs"):
            assert torch.equal(first[k], again[k]), (i, k)


def test_fallbacks_run_the_unfused_launches(dev, monkeypatch):
    """With fewer CUs left than tiles (devit_set_reserved_cus) a workgroup would get a second tile, whose prefetched stages fill the LDS the epilogue
    stages rows in: the two launches run instead, and give what DEVIT_LNFUSE=0 gives.  D != 384 never fuses."""
    from devit_amd import _lib as L
    from devit_amd._lib import call
    lib = L.load()
    inp = make_inputs(dev, 256, 1536, 8)
    tiles = inp["Mp"] // 256
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    monkeypatch.setenv("DEVIT_LNFUSE", "0")
    ref = launch(inp)
    monkeypatch.delenv("DEVIT_LNFUSE")
    assert lib.devit_dgrad_layernorm_bwd_fused(inp["Mp"], 768, 1536) == 0
    before = lib.devit_get_reserved_cus()
    reserve = min(128, (cus - tiles) // 8 * 8 + 8)
    assert cus - reserve < tiles <= cus - before, (cus, tiles, before)
    try:
        call("devit_set_reserved_cus", reserve)
        assert lib.devit_dgrad_layernorm_bwd_fused(inp["Mp"], D, 1536) == 0
        got = launch(inp)
    finally:
        call("devit_set_reserved_cus", before)
    assert got["wrote_dln"]
    for k in ("dln", "dx", "dxb"):
        assert torch.equal(ref[k], got[k]), k
    check_column_sums(inp, ref, got)                 # (the same kernels on a smaller GEMM grid: the LayerNorm launches are the same)
    assert lib.devit_dgrad_layernorm_bwd_fused(inp["Mp"], D, 1536) == 1
    assert not launch(inp)["wrote_dln"]


def test_training_step_with_and_without_fusion_full_size(dev, monkeypatch):
    """bs-256 training forward + backward through the model (devit_block_bwd takes the fused launch at both sites of every block) with
    DEVIT_LNFUSE=0 and =1: logits and q / k / v of block 5 identical; the gradient of pos_embed (behind every dgrad and every LayerNorm backward)
    to 1e-5 of its maximum, as tests/test_gpu_fullsize.py holds the full-row kernel; every parameter's gradient within 2e-5 of its largest
    element (weight gradients are fp32 atomics, the LayerNorm / bias gradients are summed in another order)."""
    import devit_amd
    torch.manual_seed(5)
    s = devit_amd.create_model("dedeit", num_classes=25, drop_path_rate=0.1).to(dev).train()
    g = torch.Generator(device=dev).manual_seed(34)
    img = torch.randn((256, 3, 224, 224), generator=g, device=dev)

    def run(flag):
        monkeypatch.setenv("DEVIT_LNFUSE", flag)
        for p in s.parameters():
            p.grad = None
        torch.manual_seed(11)                      # the same DropPath masks in both runs
        out = s(img, output_qkv=True)
        lg = out["output"][0]
        q, k, v = out["qkv"][5]
        (lg.float().square().mean() + q.float().mean() + v.float().square().mean()).backward()
        torch.cuda.synchronize()
        return (lg.detach().clone(), q.detach().clone(), k.detach().clone(), v.detach().clone()), {n: p.grad.detach().clone() for n, p in s.named_parameters() if p.grad is not None}

    (ref_out, ref_g), (got_out, got_g) = run("0"), run("1")
    for a, b in zip(ref_out, got_out):
        assert torch.equal(a, b)
    pe = float((ref_g["pos_embed"] - got_g["pos_embed"]).abs().max()) / float(ref_g["pos_embed"].abs().max())
    print(f"pos_embed.grad: {pe:.3e} of its maximum")
    assert pe <= 1e-5
    assert set(ref_g) == set(got_g) and len(ref_g) > 12 * 12      # (this loss leaves the distillation head without a gradient)
    worst = ("", 0.0)
    for n in ref_g:
        e = float((ref_g[n] - got_g[n]).abs().max()) / max(float(ref_g[n].abs().max()), 1e-30)
        worst = max(worst, (n, e), key=lambda t: t[1])
        assert e <= 2e-5, (n, e)
    print(f"largest parameter-gradient difference: {worst[1]:.3e} of its largest element ({worst[0]})")
