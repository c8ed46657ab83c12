"""Properties at BASELINE.json's FULL sizes (B = 256, N = 198 -> M = 50688 token rows), where a CPU oracle run would take
minutes: exact integer arithmetic through the bf16 MFMA path (every product and partial sum representable, so the result
must equal the integer matmul bit for bit), linearity, softmax row sums, LayerNorm statistics, and bit-reproducibility
of the student / teacher forward; the BACKWARD kernels at their full grids (attention 1536 workgroups, LayerNorm 50688
rows) against torch fp32 autograd on image slices; and the whole bs-256 DEKD step in bf16 against the same step on the
exact-fp32 path (which test_gpu_model.py pins to the reference goldens at 2e-6).  The bs-8 comparisons with the oracle
and the goldens are in test_gpu_model.py."""
import pytest
import torch

from conftest import chk

pytestmark = pytest.mark.gpu
BF16, F32 = torch.bfloat16, torch.float32
B, N = 256, 198
M = B * N


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda")


def ints(shape, lo, hi, dev, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, generator=g).to(dev)


# The last three shapes are the teacher's fc2 (residual epilogue without a DropPath scale, with the bf16 branch copy), the same
# shape with a plain fp32 store, and fc1's shape: 256x256-tile launches of 2.32 and 9.28 rounds on 256 CUs.
@pytest.mark.parametrize("Nout,K,kind,bkm", [
    (1152, 384, "f32", 0), (2304, 768, "bf16", 0), (768, 3072, "res", 0), (384, 1536, "f32", 1), (1536, 384, "bf16", 0),
    (768, 3072, "res_noscale", 0), (768, 3072, "f32", 0), (3072, 768, "bf16", 0),
    # the full-row 256x384 kernel (k-major weight, N = 384): qkv's dgrad shape with the bf16 store, fc2's forward with the residual epilogue
    (384, 1152, "bf16", 1), (384, 1536, "res", 1)])
def test_gemm_exact_integers_full_size(dev, Nout, K, kind, bkm):
    """A in {-3..3}, W in {-1,0,1}: |sum| <= 3 K < 2^14, exact in fp32 and (for the bf16 store: values clipped to
    |x| <= 256 by construction of a sparse W) in bf16 -- every output tile of the persistent launch, bit for bit."""
    from devit_amd import ops, _lib as L
    a = ints((M, K), -3, 3, dev, 1).to(BF16)
    w = ints((K, Nout) if bkm else (Nout, K), -1, 1, dev, 2)
    if kind == "bf16":                          # keep |sum| <= 255 so that the bf16 store is exact: sparse W
        w = w * (ints(w.shape, 0, K // 32 - 1, dev, 3) == 0)
        assert int(w.abs().sum(0 if bkm else 1).max()) * 3 <= 255
    w = w.to(BF16)
    ref = a.float() @ (w.float() if bkm else w.float().t())
    if kind == "f32":
        out = torch.empty((M, Nout), dtype=F32, device=dev)
        ops.gemm(a, K, 0, w, Nout if bkm else K, bkm, M, Nout, K, kind=L.EPI_STORE_F32, out=out, ldc=Nout)
        assert torch.equal(out, ref)
    elif kind == "bf16":
        out = torch.empty((M, Nout), dtype=BF16, device=dev)
        ops.gemm(a, K, 0, w, Nout if bkm else K, bkm, M, Nout, K, kind=L.EPI_STORE_BF16, out=out, ldc=Nout)
        assert torch.equal(out.float(), ref)
    elif kind == "res_noscale":                 # the teacher's fc2 (eval: no DropPath scale), bf16 copy of the branch too
        res = ints((M, Nout), -50, 50, dev, 4).float()
        out = torch.empty((M, Nout), dtype=F32, device=dev)
        copy = torch.empty((M, Nout), dtype=BF16, device=dev)
        ops.gemm(a, K, 0, w, K, 0, M, Nout, K, kind=L.EPI_RESIDUAL_F32, out=out, ldc=Nout, res=res, aux=copy)
        assert torch.equal(out, res + ref)
        exact = ref.abs() <= 256                # integers up to 256 are bf16 values: the branch copy is exact there
        assert torch.equal(copy.float()[exact], ref[exact]) and float(exact.float().mean()) > 0.99
    else:                                       # residual epilogue with a per-image scale in {0, 1, 2}
        res = ints((M, Nout), -50, 50, dev, 4).float()
        rs = ints((B,), 0, 2, dev, 5).float()
        out = torch.empty((M, Nout), dtype=F32, device=dev)
        ops.gemm(a, K, 0, w, Nout if bkm else K, bkm, M, Nout, K, kind=L.EPI_RESIDUAL_F32, out=out, ldc=Nout, res=res, rowscale=rs,
                 rows_per_scale=N)
        assert torch.equal(out, res + rs.repeat_interleave(N)[:, None] * ref)


def test_wgrad_exact_and_linear_full_size(dev):
    """dW = dY^T X over all 50688 rows with split-K atomics: integer operands -> the fp32 atomic sum is exact whatever
    the order; and the accumulate-into-existing-content contract (two calls add)."""
    from devit_amd import ops, _lib as L
    Nw, K = 1536, 384
    dy, x = ints((M, Nw), -2, 2, dev, 6).to(BF16), ints((M, K), -2, 2, dev, 7).to(BF16)
    ref = dy.float().t() @ x.float()                                  # |sum| <= 4 * 50688 < 2^24: exact
    out = torch.zeros((Nw, K), dtype=F32, device=dev)
    for _ in range(2):
        ops.gemm(dy, Nw, 1, x, K, 1, Nw, K, M, kind=L.EPI_ATOMIC_F32, out=out, ldc=K, split_k=ops.split_k_for(Nw, K, M // 64))
    assert torch.equal(out, 2 * ref)


def test_grouped_wgrads_exact_and_linear_full_size(dev):
    """The step's weight gradients as the step launches them (round 6): ONE launch of the grouped full-row kernel over the products of eleven
    blocks at all 50688 rows (44 jobs, 209 tiles, no K split) and one block's four products alone (13 K slices of atomics).  Integer operands:
    every product and every fused bias gradient is exact whatever the order of the adds; two launches add (accumulate-into-`.grad` contract)."""
    from devit_amd import ops
    D, Hd, NB = 384, 1536, 11
    shapes = ((3 * D, D), (D, D), (Hd, D), (D, Hd))
    sets = [[(ints((M, n), -2, 2, dev, 40 + 10 * s + i).to(BF16), ints((M, k), -2, 2, dev, 60 + 10 * s + i).to(BF16)) for i, (n, k) in enumerate(shapes)]
            for s in range(2)]                                        # two blocks' operands, used alternately
    refs = [[dy.float().t() @ x.float() for dy, x in st] for st in sets]
    gw = [[torch.zeros(sh, dtype=F32, device=dev) for sh in shapes] for _ in range(NB)]
    gb = [[torch.zeros(sh[0], dtype=F32, device=dev) for sh in shapes] for _ in range(NB)]
    jobs = [(sets[l & 1][i][0], sets[l & 1][i][1], gw[l][i], gb[l][i] if i != 3 else None) for l in range(NB) for i in range(4)]
    for _ in range(2):
        ops.linear_wgrads(jobs, M)
    for l in range(NB):
        for i in range(4):
            assert torch.equal(gw[l][i], 2 * refs[l & 1][i]), (l, i)
            if i != 3:
                assert torch.equal(gb[l][i], 2 * sets[l & 1][i][0].float().sum(0)), (l, i)
    one = [torch.zeros(sh, dtype=F32, device=dev) for sh in shapes]
    ops.linear_wgrads([(sets[0][i][0], sets[0][i][1], one[i], None) for i in range(4)], M)      # 19 tiles x 13 slices
    for i in range(4):
        assert torch.equal(one[i], refs[0][i]), i


def test_attention_rows_sum_to_gate_full_size(dev):
    """V = 1 everywhere -> every output element is gate_h * sum_j P_ij = gate_h (P is rounded to bf16 before P V, so to
    2^-8); and the log-sum-exp of a constant score row is log N + the score."""
    from devit_amd import ops
    from devit_amd._lib import call, ptr, stream_ptr
    H, D = 6, 384
    qkv = ops.rows_alloc(M, 3 * D, BF16, dev)
    g = torch.Generator(device="cpu").manual_seed(8)
    qkv[:M, : 2 * D] = torch.randn((M, 2 * D), generator=g).to(dev).to(BF16)
    qkv[:M, 2 * D:] = 1.0
    gate = torch.tensor([1.0, 0.0, 0.5, 1.0, 2.0, 1.0], device=dev)
    out = ops.rows_alloc(M, D, BF16, dev)
    lse = torch.empty((B, H, N), dtype=F32, device=dev)
    call("devit_attn_fwd", ptr(qkv), ptr(out), ptr(lse), ptr(gate), B, N, H, 64, 0.125, 0, stream_ptr())
    o = out[:M].float().view(M, H, 64)
    assert float((o - gate.view(1, H, 1)).abs().max()) < 2 ** -7 * 2.0
    qkv[:M, : 2 * D] = 0.0                                            # all scores 0 -> lse = log N exactly-ish
    call("devit_attn_fwd", ptr(qkv), ptr(out), ptr(lse), ptr(gate), B, N, H, 64, 0.125, 0, stream_ptr())
    assert float((lse - torch.log(torch.tensor(float(N)))).abs().max()) < 1e-5


def test_layernorm_statistics_full_size(dev):
    from devit_amd import ops
    for D in (384, 768):
        g = torch.Generator(device="cpu").manual_seed(9)
        x = (torch.randn((M, D), generator=g) * 3 + 1.5).to(dev)
        y = torch.empty((M, D), dtype=F32, device=dev)
        mean, rstd = torch.empty(M, device=dev), torch.empty(M, device=dev)
        ops.layernorm_fwd(x, M, D, torch.ones(D, device=dev), torch.zeros(D, device=dev), 1e-6, y_f32=y, mean=mean, rstd=rstd)
        assert float(y.mean(1).abs().max()) < 1e-5 and float((y.var(1, unbiased=False) - 1).abs().max()) < 1e-4
        assert float((mean - x.mean(1)).abs().max()) < 1e-5
        assert float((rstd - torch.rsqrt(x.var(1, unbiased=False) + 1e-6)).abs().max()) < 1e-4


def test_forward_bit_reproducible_full_size(dev):
    """bs-256 student (train, fixed DropPath masks) and teacher (eval) forwards twice: no atomics, no data-dependent
    order on the forward path -> identical bits; logits finite; teacher/student agree in shape with the loss kernels."""
    import devit_amd
    from devit_amd import engine
    torch.manual_seed(0)
    s = devit_amd.create_model("dedeit", num_classes=25, drop_path_rate=0.1, drop_block_rate=None).to(dev).train()
    t = devit_amd.create_model("deit_base_distilled_patch16_224", num_classes=25).to(dev).eval()
    img = torch.randn((B, 3, 224, 224), generator=torch.Generator(device="cpu").manual_seed(10)).to(dev)
    dps = [(torch.ones(B, device=dev), torch.full((B,), 1.0 / 0.9, device=dev) * (torch.arange(B, device=dev) % 10 != 0))
           for _ in range(12)]
    with torch.no_grad():
        a1 = engine._forward_with_dp(s, img, dps)["output"]
        a2 = engine._forward_with_dp(s, img, dps)["output"]
        b1, b2 = t(img), t(img)
    assert torch.equal(a1[0], a2[0]) and torch.equal(a1[1], a2[1]) and torch.equal(b1, b2)
    assert bool(torch.isfinite(a1[0]).all()) and bool(torch.isfinite(b1).all()) and b1.shape == (B, 25)


# ------------------------------------------------------------------------------------------ backward at full size
def relmax(a, b):
    return float((a.float() - b.float()).abs().max() / b.float().abs().max().clamp_min(1e-30))


@pytest.mark.parametrize("H,with_add", [(6, True), (12, False)])
def test_attention_backward_full_size(dev, H, with_add):
    """attn_bwd_kernel on its full grid (B x H = 1536 / 3072 workgroups, one per CU at 152 KB of LDS): dq/dk/dv of three
    16-image slices (first, middle, last images) against torch fp32 autograd of softmax attention on the same bf16
    inputs; the relation-loss gradient that the student's middle block adds in is checked on the student shape."""
    from devit_amd import ops
    from devit_amd._lib import call, ptr, stream_ptr
    from _attn_model import check_packed
    from conftest import chk
    D = H * 64
    g = torch.Generator(device=dev).manual_seed(11 + H)
    qkv = ops.rows_alloc(M, 3 * D, BF16, dev)
    qkv[:M] = (torch.randn((M, 3 * D), generator=g, device=dev) * 0.8).to(BF16)
    gate = torch.ones(H, device=dev)
    gate[1], gate[2] = 0.0, 0.5
    out = ops.rows_alloc(M, D, BF16, dev)
    lse = torch.empty((B, H, N), dtype=F32, device=dev)
    call("devit_attn_fwd", ptr(qkv), ptr(out), ptr(lse), ptr(gate), B, N, H, 64, 0.125, 0, stream_ptr())
    dout = ops.rows_alloc(M, D, BF16, dev)
    dout[:M] = torch.randn((M, D), generator=g, device=dev).to(BF16)
    add = None
    if with_add:
        add = ops.rows_alloc(M, 3 * D, BF16, dev)
        add[:M] = (torch.randn((M, 3 * D), generator=g, device=dev) * 0.5).to(BF16)
    dqkv = ops.rows_alloc(M, 3 * D, BF16, dev)
    call("devit_attn_bwd", ptr(qkv), ptr(out), ptr(dout), ptr(lse), ptr(gate), ptr(add), ptr(dqkv), B, N, H, 64, 0.125,
         stream_ptr())
    assert bool(torch.isfinite(dqkv[:M].float()).all())
    for b0 in (0, 120, B - 16):
        r0, r1 = b0 * N, (b0 + 16) * N
        x = qkv[r0:r1].float().requires_grad_(True)
        v = x.view(16, N, 3, H, 64).permute(2, 0, 3, 1, 4)
        a = ((v[0] @ v[1].transpose(-2, -1)) * 0.125).softmax(-1)
        o = ((a @ v[2]).transpose(1, 2) * gate.view(1, 1, H, 1)).reshape(16 * N, D)
        assert relmax(out[r0:r1], o) < 1e-2
        o.backward(dout[r0:r1].float())
        ref = x.grad + (add[r0:r1].float() if add is not None else 0)
        e = relmax(dqkv[r0:r1], ref)
        assert e < 2e-2, f"images {b0}..{b0 + 16}: dqkv rel-to-max err {e:.3e}"
        # ... and every element of O, lse, dQ, dK, dV of the slice against its own bound (tests/_attn_model.py)
        check_packed(chk, f"full_size/H{H}/images{b0}", qkv[r0:r1], 16, N, H, gate, 0.125, out[r0:r1], lse[b0:b0 + 16], dout[r0:r1], dqkv[r0:r1],
                     None if add is None else add[r0:r1])


@pytest.mark.parametrize("D", [384, 768])
def test_layernorm_backward_full_size(dev, D):
    """ln_bwd_kernel over all 50688 rows (the fused form the blocks use: bf16 dy in, residual gradient added, per-image
    DropPath scale on the bf16 copy, gamma / beta gradients, column sums of the bf16 copy): dx on three 16-image slices
    and the four full-length reductions against torch fp32 autograd."""
    from devit_amd import ops
    g = torch.Generator(device=dev).manual_seed(21 + D)
    x = torch.randn((M, D), generator=g, device=dev) * 2.0 + 0.3
    gm = 1 + 0.1 * torch.randn(D, generator=g, device=dev)
    bt = 0.1 * torch.randn(D, generator=g, device=dev)
    y = torch.empty((M, D), dtype=BF16, device=dev)
    mean, rstd = torch.empty(M, device=dev), torch.empty(M, device=dev)
    ops.layernorm_fwd(x, M, D, gm, bt, 1e-6, y_bf16=y, mean=mean, rstd=rstd)
    dy = torch.randn((M, D), generator=g, device=dev).to(BF16)
    dres = torch.randn((M, D), generator=g, device=dev)
    rsc = (torch.arange(B, device=dev) % 7 != 0).float() / 0.9
    dx = torch.empty((M, D), dtype=F32, device=dev)
    dxb = torch.empty((M, D), dtype=BF16, device=dev)
    dg, db, gs = torch.zeros(D, device=dev), torch.zeros(D, device=dev), torch.zeros(D, device=dev)
    ops.layernorm_bwd(dy, False, x, M, D, mean, rstd, gm, dres, dx, dxb, rsc, N, dg, db, gsum=gs)
    xr = x.clone().requires_grad_(True)
    gr, br = gm.clone().requires_grad_(True), bt.clone().requires_grad_(True)
    ref = torch.nn.functional.layer_norm(xr, (D,), gr, br, 1e-6)
    ref.backward(dy.float())
    want = xr.grad + dres
    for b0 in (0, 120, B - 16):
        r0, r1 = b0 * N, (b0 + 16) * N
        assert relmax(dx[r0:r1], want[r0:r1]) < 1e-5
        assert relmax(dxb[r0:r1], want[r0:r1] * rsc[b0:b0 + 16].repeat_interleave(N)[:, None]) < 2 ** -7
    assert relmax(dg, gr.grad) < 2e-4 and relmax(db, br.grad) < 2e-4      # 50688-term fp32 sums, different order
    assert relmax(gs, dxb.float().sum(0)) < 2e-4


def test_distill_step_bf16_vs_f32_full_size(dev):
    """The benchmarked step at BASELINE's size (bs 256, C = 25, DeiT-B -> dedeit), bf16 path against the exact-fp32 path
    (precision="f32": pinned to the reference goldens at 2e-6 by test_gpu_model.test_f32_path_meets_1e3_bar) on the
    same weights, inputs and DropPath masks: the five losses, every parameter's gradient norm, gradient slices of every
    kind of parameter.  This is the only place the bs-256 backward (attention / LayerNorm backward at 1536 workgroups /
    50688 rows, dGELU dgrad, split-K wgrads with fused bias gradients, relation-loss gradient) is compared with anything."""
    import devit_amd
    from devit_amd import engine
    torch.manual_seed(3)
    C = 25
    s = devit_amd.create_model("dedeit", num_classes=C, drop_path_rate=0.1, drop_block_rate=None).to(dev).train()
    t = devit_amd.create_model("deit_base_distilled_patch16_224", num_classes=C).to(dev).eval()
    for p in t.parameters():
        p.requires_grad_(False)
    g = torch.Generator(device=dev).manual_seed(31)
    img = torch.randn((B, 3, 224, 224), generator=g, device=dev)
    y1, y2 = torch.randint(0, C, (B,), generator=g, device=dev), torch.randint(0, C, (B,), generator=g, device=dev)
    oh = lambda y: torch.full((B, C), 0.1 / C, device=dev).scatter_(1, y[:, None], 0.9 + 0.1 / C)
    soft = 0.7 * oh(y1) + 0.3 * oh(y2)
    keep = torch.linspace(0, 0.1, 12)
    dps = []
    for i in range(12):
        k = 1.0 - float(keep[i])
        u = torch.rand((2, B), generator=g, device=dev)
        sc = torch.floor(k + u) / k
        dps.append((sc[0].contiguous(), sc[1].contiguous()))
    res = {}
    for prec in ("f32", "bf16"):
        s.precision = t.precision = prec
        for p in s.parameters():
            p.grad = None
        out = engine.distill_forward(s, t, img, soft, gama=(0.2, 0.1, 0.3), kind="hard", alpha=0.5, tau=1.0, dp_scales=dps)
        out["loss"].backward()
        torch.cuda.synchronize()
        res[prec] = ({k: float(out[k]) for k in ("loss", "cls_loss", "q_loss", "k_loss", "v_loss")},
                     {n: p.grad.detach().clone() for n, p in s.named_parameters()},
                     out["logits"][0].detach().clone(), out["teacher_logits"].detach().clone())
    s.precision = t.precision = "bf16"
    (l32, g32, lo32, tl32), (l16, g16, lo16, tl16) = res["f32"], res["bf16"]
    for k in l32:
        assert chk(abs(l16[k] - l32[k]) / abs(l32[k]), 2e-3), (k, l16[k], l32[k])
    assert chk(relmax(lo16, lo32), 1.5e-2) and chk(relmax(tl16, tl32), 1.5e-2)
    n32 = torch.stack([g32[n].norm() for n in g32])
    n16 = torch.stack([g16[n].norm() for n in g32])
    chk(float(((n16 - n32).abs() / (n32 + 1e-3 * n32.max())).max()), 1e-2)
    bad = (n16 - n32).abs() > 1e-2 * n32 + 1e-3 * n32.max()
    assert not bool(bad.any()), [(n, float(a), float(b)) for n, a, b, f in zip(g32, n16, n32, bad) if f][:8]
    slices = ["head.weight", "head_dist.bias", "norm.weight", "blocks.11.mlp.fc2.weight", "blocks.11.mlp.fc2.bias",
              "blocks.7.mlp.fc1.weight", "blocks.7.mlp.fc1.bias", "blocks.5.attn.qkv.weight", "blocks.5.attn.qkv.bias",
              "blocks.5.attn.proj.weight", "blocks.2.norm1.weight", "blocks.0.norm2.bias", "blocks.0.attn.proj.bias",
              "patch_embed.proj.weight", "patch_embed.proj.bias", "pos_embed", "cls_token", "dist_token"]
    worst = {}
    for n in slices:
        e = relmax(g16[n], g32[n])
        worst[n] = e
        # measured on MI355X (profiles/r02_parity_margins.json): weight matrices <= 2.1e-2 of their largest element, the 1-D
        # LayerNorm / bias gradients (sums over 50688 rows of bf16-rounded products) <= 2.2e-2; the patch-embedding
        # weights sit behind all twelve blocks' backward and carry the most (4.2e-2)
        bar = 7e-2 if n.startswith(("patch_embed", "pos_embed", "cls_token", "dist_token")) else (3e-2 if g32[n].ndim > 1 else 4e-2)
        assert chk(e, bar), f"{n}: gradient rel-to-max err {e:.3e}"
    print("bs-256 bf16 vs f32 gradient slices, rel-to-max:", {k: round(v, 5) for k, v in worst.items()})


def test_full_row_gemm_inside_the_model_full_size(dev, monkeypatch):
    """The student's fc2 forward and its qkv / proj / fc1 dgrads run on the full-row 256x384 GEMM (csrc/gemmfr.hip, default at >= 64 row tiles);
    fc2 reads a K-MAJOR copy of its weight that must follow every rewrite of the bf16 copy.  At bs 256: the training forward + backward with the
    kernel switched off (DEVIT_GEMMFR=0) and on -- logits and q / k / v of the middle block bit-identical, the gradient of pos_embed (behind every
    dgrad) to fp32 round-off (the weight gradients go through fp32 atomics: not compared) -- and again after an optimizer step of the fused flat AdamW, which rewrites the bf16 copies
    in place: a stale k-major copy would show as different logits."""
    import devit_amd
    from devit_amd import ddp, optim
    torch.manual_seed(5)
    s = devit_amd.create_model("dedeit", num_classes=25, drop_path_rate=0.0).to(dev).train()
    flat = ddp.FlatParams(s)
    flat.attach_bf16(s)
    opt = optim.FlatAdamW(flat, lr=1e-3, weight_decay=0.05, max_norm=1.0, ema_decay=None)
    g = torch.Generator(device=dev).manual_seed(32)
    img = torch.randn((B, 3, 224, 224), generator=g, device=dev)

    def run(flag):
        monkeypatch.setenv("DEVIT_GEMMFR", flag)
        opt.zero_grad()
        out = s(img, output_qkv=True)
        lg = out["output"][0]                     # (class-token logits, distillation-token logits) in training mode
        q, k, v = out["qkv"][5]
        (lg.float().square().mean() + q.float().mean() + v.float().square().mean()).backward()
        torch.cuda.synchronize()
        return lg.detach().clone(), q.detach().clone(), k.detach().clone(), v.detach().clone(), s.pos_embed.grad.detach().clone()

    for phase in range(2):
        ref = run("0")
        got = run("1")
        for a, b in zip(ref[:4], got[:4]):
            assert torch.equal(a, b), phase
        # the gradient that reaches the embedding went through every dgrad of every block (a sum over the batch: compared to fp32 round-off)
        assert float((ref[4] - got[4]).abs().max()) <= 1e-5 * float(ref[4].abs().max()), phase
        opt.step()          # rewrites masters + bf16 copies in place; the k-major copies must follow
    monkeypatch.setenv("DEVIT_GEMMFR", "1")
    s.eval()
    with torch.no_grad():
        a = s(img[:128])
        monkeypatch.setenv("DEVIT_GEMMFR", "0")
        b = s(img[:128])
    assert torch.equal(a, b)


def test_full_row_gemm_through_compacted_blocks_full_size(dev, monkeypatch):
    """The same identity for a physically shrunk student (shrink.compact(trainable=True), 0.3 / 0.3 gates): the compact fc2 weight [384][1152]
    gets its k-major copy behind every re-gather (a second launch), fc1's dgrad runs at K = 1152 and qkv's at K = 768 on the full-row kernel."""
    import devit_amd
    from devit_amd import shrink
    torch.manual_seed(6)
    s = devit_amd.create_model("dedeit", num_classes=25, drop_path_rate=0.0).to(dev).train()
    gen = torch.Generator().manual_seed(7)
    for blk in s.blocks:
        hm, nm = torch.ones(6), torch.ones(1536)
        hm[torch.randperm(6, generator=gen)[:2]] = 0
        nm[torch.randperm(1536, generator=gen)[:461]] = 0
        blk.attn.gate, blk.mlp.gate = hm, nm
    shrink.compact(s, trainable=True)
    try:
        assert s.blocks[0]._compact["fc2_w16t"].shape == (1152, 384)
        g = torch.Generator(device=dev).manual_seed(33)
        img = torch.randn((B, 3, 224, 224), generator=g, device=dev)

        def run(flag):
            monkeypatch.setenv("DEVIT_GEMMFR", flag)
            for p in s.parameters():
                p.grad = None
            out = s(img, output_qkv=True)
            lg = out["output"][0]
            (lg.float().square().mean() + out["qkv"][5][2].float().square().mean()).backward()
            torch.cuda.synchronize()
            return lg.detach().clone(), s.pos_embed.grad.detach().clone()

        ref, got = run("0"), run("1")
        assert torch.equal(ref[0], got[0])
        assert float((ref[1] - got[1]).abs().max()) <= 1e-5 * float(ref[1].abs().max())
        with torch.no_grad():                      # move a master: the next forward re-gathers AND re-transposes
            s.blocks[3].mlp.fc2.weight.mul_(1.25)
        ref, got = run("0"), run("1")
        assert torch.equal(ref[0], got[0])
    finally:
        shrink.uncompact(s)


def test_ensemble_config5_full_size(dev):
    """BASELINE config 5 at its size: four `dedeit` sub-models (250 classes each, shrink_ratio 0.3 head / neuron gates) +
    EnsMLP -> 1000 classes, bs 256, inference (ensemble.py; models/ensemble_models.py:32-40).  The 4 x 25-class, bs-4 form is
    held to the reference golden (test_gpu_model.py::test_ensemble_vs_golden); here, where a CPU run would take minutes:
      * the physically shrunk models (shrink.compact) compute the masked models' function,
      * uncompact restores the masked outputs bit for bit,
      * the first 8 images of the bs-256 batch give what a bs-8 batch of the same images gives (every kernel is row- or
        image-local and a tile's K order does not depend on M), which ties this size to the oracle-checked small cases."""
    import devit_amd
    from devit_amd import shrink
    from devit_amd.ensemble_models import EnsMLP, MultiViT
    torch.manual_seed(5)
    multi = MultiViT("dedeit", drop=0, drop_path=0.0, num_classes_list=[250] * 4, num_div=4).to(dev).eval()
    ens = EnsMLP("dedeit", 1000, 384, [250] * 4, 768).to(dev).eval()
    g = torch.Generator().manual_seed(0)
    for bb in multi.backbones:
        for blk in bb.blocks:
            hm = torch.ones(6); hm[torch.randperm(6, generator=g)[:2]] = 0
            nm = torch.ones(1536); nm[torch.randperm(1536, generator=g)[:461]] = 0
            blk.attn.gate, blk.mlp.gate = hm, nm
    img = torch.randn(B, 3, 224, 224, generator=torch.Generator().manual_seed(6)).to(dev)
    with torch.no_grad():
        masked = ens(multi(img))
        small = ens(multi(img[:8].contiguous()))
        assert masked.shape == (B, 1000) and bool(torch.isfinite(masked).all())
        assert torch.equal(masked[:8], small), "a batch slice must not depend on the batch it is computed in"
        rep = shrink.compact(multi)
        assert len(rep) == 4 * 12 and all(hr in (4, 6) and nr == 1152 for _, hr, _, nr in rep)
        comp = ens(multi(img))
        shrink.uncompact(multi)
        again = ens(multi(img))
    assert torch.equal(again, masked)
    # Same bf16 path with the zero terms left out: the fp32 sums group differently, which now and then moves a stored bf16
    # activation by one ulp.  Measured 3.9e-3 of max|logit| (a max over 256 000 logits).  No top-1 threshold: an argmax can
    # only flip where the top-2 margin is below twice this deviation, so agreement (253 of 256 here, random-init logits are
    # nearly flat) says how flat the logits are, not how good the kernels are -- the bound below is the whole statement.
    err = float((comp.float() - masked.float()).abs().max() / masked.float().abs().max())
    assert chk(err, 1e-2), err
