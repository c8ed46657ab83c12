"""The fused q/k/v relation loss (csrc/relation.hip: devit_relation_fused_fwd / _bwd behind ops.RelationLossFn) on a real MI355X: against
float64 inside the per-element bound the unfused launches are held to (_attn_model.relation_bounds, _tail_model.rel_feature_loss_bounds),
against the unfused launches (DEVIT_RELFUSE=0), and the properties a fused kernel can lose: masking of the rows behind an image, the extent of
what it writes, run-to-run identity, routing, and one bs-8 distillation step through the engine both ways."""
import pytest
import torch

from conftest import chk

pytestmark = pytest.mark.gpu

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
# one tile | a tile boundary | a ragged second tile | the real shape (198 = 12 x 16 + 6) | the full 208 rows | the compacted student's width
SHAPES = [(1, 5, 64, 64), (2, 16, 64, 128), (2, 17, 128, 256), (3, 198, 384, 768), (2, 208, 384, 768), (2, 198, 256, 768)]
WEIGHTS = [(0.2 / 12, 0.1 / 12, 0.3 / 12), (0.2 / 12, -0.1 / 12, 0.3 / 12)]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from devit_amd import _lib
    _lib.require_device(torch.zeros(1, device="cuda"))
    return torch.device("cuda")


def rnd(shape, dev, std, seed, dtype):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(shape, generator=g) * std).to(dev).to(dtype)


def buffers(dev, B, N, Ds, Dt, std, t_dtype=BF16, fill=0.0):
    """packed student / teacher buffers with 256 rows behind the B N live ones (what the unfused Gram windows need), those rows = fill"""
    from devit_amd import ops
    M = B * N
    s = ops.rows_alloc(M, 3 * Ds, BF16, dev, extra=256)
    t = ops.rows_alloc(M, 3 * Dt, t_dtype, dev, extra=256)
    s[:M] = rnd((M, 3 * Ds), dev, std, 1, BF16)
    t[:M] = rnd((M, 3 * Dt), dev, std, 2, t_dtype)
    s[M:] = fill
    t[M:] = fill
    return s, t


def run(s, t, B, N, wts):
    from devit_amd import ops
    s = s.detach().clone().requires_grad_(True)
    losses = ops.RelationLossFn.apply(s, t, B, N, 64, 64)
    (losses * torch.tensor(wts, device=s.device)).sum().backward()
    return losses.detach(), s.grad[:B * N].clone()


def unfused_runs(s, B, N, Ds):
    """does devit_gemm_bf16 take the three batched products of the unfused path at this student width?  (its own rule, asked)"""
    from devit_amd import ops
    L = ops.L
    gram = ops.gemm_route(s, 3 * Ds, 0, s, 3 * Ds, 0, 256, 256, Ds, kind=L.EPI_STORE_F32, out=s, ldc=256, batch=B, a_bs=N * 3 * Ds,
                          b_bs=N * 3 * Ds, out_bs=65536)
    df = ops.gemm_route(s, 256, 0, s, 3 * Ds, 1, 256, Ds, 256, kind=L.EPI_STORE_BF16, out=s, ldc=3 * Ds, batch=B, a_bs=65536,
                        b_bs=N * 3 * Ds, out_bs=N * 3 * Ds, m_valid=N)
    return gram > 0 and df > 0


def bits(x):
    return x.contiguous().view(torch.int16 if x.element_size() == 2 else torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


_REF = {}


def reference(s, t, B, N, Ds, Dt, key):
    """float64 gradient per unit weight, its bound per unit |weight| and the loss with its bound, per component: computed once per input"""
    from _attn_model import relation_bounds
    from _tail_model import rel_feature_loss_bounds
    if key not in _REF:
        M, out = B * N, []
        for j in range(3):
            fs = s[:M, j * Ds:(j + 1) * Ds].double().view(B, N, Ds)
            ft = t[:M, j * Dt:(j + 1) * Dt].double().view(B, N, Dt)
            want, bound, _ = relation_bounds(fs, ft, 1.0, 64, 64)
            out.append((want, bound) + tuple(rel_feature_loss_bounds(fs, ft, 64, 64)))
        _REF[key] = out
    return _REF[key]


def check(tag, losses, d, ref, wts, B, N, Ds):
    from _attn_model import ratio
    worst = 0.0
    for j in range(3):
        want, bound, want_l, e_l = ref[j]
        r = ratio(d[:, j * Ds:(j + 1) * Ds].double().view(B, N, Ds), want * wts[j], bound * abs(wts[j]))     # (dF and its bound are homogeneous in the weight)
        rl = ratio(losses[j].double().cpu(), want_l, e_l)
        print(f"{tag} block {j}: d worst |err| / bound {r:.3f}   loss {float(losses[j]):.6e} float64 {float(want_l):.6e} |err| / bound {rl:.3f}")
        assert chk(r, 1.0, name=f"{tag}/block{j}"), (tag, j, r)
        assert chk(rl, 1.0, name=f"{tag}/loss{j}"), (tag, j, rl)
        worst = max(worst, r)
    return worst


@pytest.mark.parametrize("B,N,Ds,Dt", SHAPES)
def test_fused_and_unfused_against_float64(dev, monkeypatch, B, N, Ds, Dt):
    """Both paths on the same buffers inside the same bounds (d per element, the three losses); their mutual difference is printed."""
    from devit_amd import ops
    for std in (0.25, 1.0):
        s, t = buffers(dev, B, N, Ds, Dt, std)
        ref = reference(s, t, B, N, Ds, Dt, (B, N, Ds, Dt, std, "bf16"))
        for wi, wts in enumerate(WEIGHTS):
            monkeypatch.delenv("DEVIT_RELFUSE", raising=False)
            assert ops.relation_fused_selected(s, t, B, N)
            lf, df = run(s, t, B, N, wts)
            check(f"relfused/{B}x{N}x{Ds}x{Dt}/std{std}/w{wi}", lf, df, ref, wts, B, N, Ds)
            monkeypatch.setenv("DEVIT_RELFUSE", "0")
            assert not ops.relation_fused_selected(s, t, B, N)
            if not unfused_runs(s, B, N, Ds):
                assert Ds < 128
                continue              # (a 64-wide student: the batched GEMM behind the unfused backward has no 64-column tile -- only the fused path exists)
            lu, du = run(s, t, B, N, wts)
            check(f"relunfused/{B}x{N}x{Ds}x{Dt}/std{std}/w{wi}", lu, du, ref, wts, B, N, Ds)
            dd = float((df.float() - du.float()).abs().max() / du.float().abs().max().clamp_min(1e-30))
            dl = float(((lf - lu).abs() / lu.abs().clamp_min(1e-30)).max())
            print(f"fused vs unfused {B}x{N}x{Ds}x{Dt} std {std} w{wi}: d max |diff| / max |d| {dd:.3e}, losses rel {dl:.3e}")
            chk(dd, 1.0, name=f"relfused_vs_unfused/{B}x{N}x{Ds}x{Dt}/std{std}/w{wi}/d")        # recorded, not asserted


def test_f16_teacher_runs_fused(dev, monkeypatch):
    """--teacher-precision f16: the teacher Gram runs on the f16 MFMA inside the fused kernel (no fallback)."""
    from devit_amd import ops
    monkeypatch.delenv("DEVIT_RELFUSE", raising=False)
    B, N, Ds, Dt = 2, 198, 384, 768
    s, t = buffers(dev, B, N, Ds, Dt, 0.25, t_dtype=F16)
    assert ops.relation_fused_selected(s, t, B, N)
    ref = reference(s, t, B, N, Ds, Dt, (B, N, Ds, Dt, 0.25, "f16"))
    lf, df = run(s, t, B, N, WEIGHTS[0])
    check("relfused/f16teacher", lf, df, ref, WEIGHTS[0], B, N, Ds)


def test_rows_behind_an_image_are_never_read(dev, monkeypatch):
    from devit_amd import ops
    monkeypatch.delenv("DEVIT_RELFUSE", raising=False)
    for B, N, Ds, Dt in ((2, 198, 384, 768), (2, 17, 128, 256)):
        s0, t0 = buffers(dev, B, N, Ds, Dt, 0.25)
        sn, tn = buffers(dev, B, N, Ds, Dt, 0.25, fill=float("nan"))
        assert ops.relation_fused_selected(sn, tn, B, N) and bool(torch.isnan(sn[B * N:]).all())
        l0, d0 = run(s0, t0, B, N, WEIGHTS[0])
        ln, dn = run(sn, tn, B, N, WEIGHTS[0])
        assert bool(torch.isfinite(l0).all()) and torch.equal(l0, ln) and torch.equal(d0, dn)
        # image 1 changed: image 0's rows of d keep their bits
        s1, t1 = s0.clone(), t0.clone()
        s1[N:2 * N] = rnd((N, 3 * Ds), dev, 0.5, 7, BF16)
        t1[N:2 * N] = rnd((N, 3 * Dt), dev, 0.5, 8, BF16)
        l1, d1 = run(s1, t1, B, N, WEIGHTS[0])
        assert torch.equal(d0[:N], d1[:N]) and not torch.equal(d0[N:], d1[N:]) and not torch.equal(l0, l1)


def test_extent_of_the_writes(dev):
    """The entry points themselves on a student buffer wider than 3 Ds: d's rows >= B N and columns >= 3 Ds, and the bytes behind S, keep their canaries;
    every element of S and of d's live block is written."""
    from devit_amd._lib import call, ptr, stream_ptr
    for B, N, Ds, Dt in ((2, 198, 256, 768), (1, 5, 64, 64)):
        M, ld_s, ld_d = B * N, 3 * Ds + 64, 3 * Ds + 8
        s = rnd((M, ld_s), dev, 0.25, 1, BF16)
        t = rnd((M, 3 * Dt), dev, 0.25, 2, BF16)
        n_s = 3 * B * 208 * 224
        S = torch.full((n_s + 4096,), 7.0, dtype=BF16, device=dev)
        stats = torch.full((3, 3, M + 64), -777.0, dtype=F32, device=dev)
        losses = torch.full((4,), 3.0, dtype=F32, device=dev)
        d = torch.full((M + 32, ld_d), 9.0, dtype=BF16, device=dev)
        up = torch.tensor([0.2, -0.1, 0.3, 11.0], dtype=F32, device=dev)
        call("devit_relation_fused_fwd", ptr(s), ptr(t), B, N, Ds, Dt, ld_s, 3 * Dt, 64, 64, 0, ptr(stats[0]), ptr(stats[1]), ptr(stats[2]),
             ptr(S), ptr(losses), stream_ptr())
        call("devit_relation_fused_bwd", ptr(S), ptr(s), ptr(up), B, N, Ds, ld_s, ptr(d), ld_d, stream_ptr())
        torch.cuda.synchronize()
        assert bool((S[n_s:] == 7.0).all()) and not bool((S[:n_s] == 7.0).any())
        Sv = S[:n_s].view(3, B, 208, 224)
        assert float(Sv[:, :, N:].abs().max()) == 0.0 and float(Sv[:, :, :, N:].abs().max()) == 0.0 and float(Sv[:, :, :N, :N].abs().max()) > 0.0
        assert float(losses[3]) == 3.0 and bool(torch.isfinite(losses[:3]).all())
        # the three statistics are [3][B N] each, packed behind their own pointers
        for k in range(3):
            flat = stats[k].flatten()
            assert not bool((flat[:3 * M] == -777.0).any()) and bool((flat[3 * M:] == -777.0).all())
        assert bool((d[M:] == 9.0).all()) and bool((d[:, 3 * Ds:] == 9.0).all()) and not bool((d[:M, :3 * Ds] == 9.0).any())


def test_five_runs_same_bits(dev, monkeypatch):
    monkeypatch.delenv("DEVIT_RELFUSE", raising=False)
    B, N, Ds, Dt = 3, 198, 384, 768
    s, t = buffers(dev, B, N, Ds, Dt, 0.25)
    first = run(s, t, B, N, WEIGHTS[1])
    for _ in range(4):
        again = run(s, t, B, N, WEIGHTS[1])
        assert same_bits(first[0], again[0]) and same_bits(first[1], again[1])


def test_routing(dev, monkeypatch):
    """N = 209, a width of 96 and an fp32 teacher buffer are not the fused kernel's: the unfused launches run, with the bits DEVIT_RELFUSE=0 gives."""
    from devit_amd import ops
    cases = [(2, 209, 128, 256, BF16), (2, 198, 96, 192, BF16), (2, 198, 128, 128, F32)]
    for B, N, Ds, Dt, t_dtype in cases:
        monkeypatch.delenv("DEVIT_RELFUSE", raising=False)
        s, t = buffers(dev, B, N, Ds, Dt, 0.25, t_dtype=t_dtype)
        assert not ops.relation_fused_selected(s, t, B, N), (B, N, Ds, Dt, t_dtype)
        if not unfused_runs(s, B, N, Ds):
            assert Ds == 96
            continue                  # (a width the batched GEMM refuses as well: nothing to run, the selection above is the check)
        a = run(s, t, B, N, WEIGHTS[0])
        monkeypatch.setenv("DEVIT_RELFUSE", "0")
        b = run(s, t, B, N, WEIGHTS[0])
        assert same_bits(a[0], b[0]) and same_bits(a[1], b[1])
    monkeypatch.setenv("DEVIT_RELFUSE", "1")
    s, t = buffers(dev, 2, 198, 384, 768, 0.25)
    assert ops.relation_fused_selected(s, t, 2, 198) and not ops.relation_fused_selected(s, t[:, :-1], 2, 198)


def test_bs8_step_through_the_engine_both_ways(dev, monkeypatch):
    """One bs-8 distill_forward + backward with the switch on and off: the total loss and the student's flat gradient inside the bars
    tests/test_gpu_trajectory.py holds the bs-8 bf16 trajectory to against its oracle (first-step loss 1e-3 relative, movement 6e-2 relative L2:
    `bars["bf16"]["step1"]`, `["mov"]` there); the measured differences are printed and recorded."""
    import devit_amd
    from devit_amd import engine
    from oracle import devit_oracle as O
    from oracle.detgen import det_array, det_labels
    C, B = 25, 8
    gs, gt = O.GEOMETRY["dedeit"], O.GEOMETRY["deit_base_distilled_patch16_224"]
    student = devit_amd.create_model("dedeit", num_classes=C, drop_path_rate=0.0)
    teacher = devit_amd.create_model("deit_base_distilled_patch16_224", num_classes=C)
    student.load_state_dict(O.make_state(gs, C, "S"))
    teacher.load_state_dict(O.make_state(gt, C, "T"))
    student.to(dev).train()
    teacher.to(dev).eval()
    img = torch.from_numpy(det_array("relfused", (B, 3, 224, 224), std=0.8)).to(dev)
    y = torch.from_numpy(det_labels("relfused_y", B, C))
    soft = (torch.nn.functional.one_hot(y, C).float() * 0.9 + 0.1 / C).to(dev)
    res = {}
    for flag in ("1", "0"):
        monkeypatch.setenv("DEVIT_RELFUSE", flag)
        student.zero_grad(set_to_none=True)
        out = engine.distill_forward(student, teacher, img, soft)
        out["loss"].backward()
        torch.cuda.synchronize()
        res[flag] = (float(out["loss"].detach()), torch.cat([p.grad.flatten().float() for p in student.parameters() if p.grad is not None]),
                     [float(out[k].detach()) for k in ("q_loss", "k_loss", "v_loss")])
    (l1, g1, r1), (l0, g0, r0) = res["1"], res["0"]
    e_loss = abs(l1 - l0) / abs(l0)
    e_grad = float((g1 - g0).norm() / g0.norm())
    print(f"bs-8 step fused vs unfused: loss {l1:.7f} / {l0:.7f} rel {e_loss:.2e}, flat gradient rel L2 {e_grad:.2e}, q/k/v {r1} / {r0}")
    assert g1.numel() == g0.numel() and float(g0.norm()) > 0
    assert chk(e_loss, 1e-3, name="relfused_bs8/loss") and chk(e_grad, 6e-2, name="relfused_bs8/grad")
