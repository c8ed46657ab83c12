"""Image sizes other than 224 on a real MI355X (img_size / --input-size; square sides 32 .. 224 in steps of the 16-pixel patch).

Kernels: the four patch-cutting kernels at S = 32 (2 x 2 patches: fewer rows than one 16-row tile), 48 (odd grid), 112 and 208 (13 x 13),
B = 1, 2, 3 (odd B: the middle sample is its own Mixup partner), bit for bit against torch's gather and ONE round-to-nearest-even cast,
every output buffer with a sentinel region behind it.  Model, lean tail and one DEKD step against the size-general CPU helper
(tests/_imgsize_model.py, pinned to the oracle and to the reference by tests/test_imgsize_host.py).

Bars are the project's own: precision="f32" logits 1e-3 of max|logit| with top-1 equal, losses 1e-4, gradient norms and slices 1e-3
(test_gpu_model.py::test_f32_path_meets_1e3_bar); bf16 logits 1.5e-2 with top-1 equal, losses 5e-4, gradient norms 3e-3, slices 1.5e-2
(::test_model_forward_vs_golden, ::test_distill_step_vs_golden).  The bf16 bars were measured at 224; what the other sizes measure goes
through conftest.chk into the session's parity_margins.json (committed rows: profiles/imgsize_parity_margins.json)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import _imgsize_model as IM
from oracle import devit_oracle as O
from oracle.detgen import det_array, det_labels
from conftest import chk

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C = 25
GS, GT = O.GEOMETRY["dedeit"], O.GEOMETRY["deit_base_distilled_patch16_224"]
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
SENTINEL, TAIL_ROWS = 7.0, 8
KERNEL_SIZES = [32, 48, 112, 208]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from devit_amd import _lib
    _lib.require_device(torch.zeros(1, device="cuda"))
    return torch.device("cuda")


def rel(a, b):
    a = a.detach().float().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    b = b.detach().float().cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


_img_cache = {}


def images(B, S):
    """(cpu, device) copies of a deterministic batch; computed once per shape, never written."""
    if (B, S) not in _img_cache:
        cpu = torch.from_numpy(det_array(f"imgsize/k{S}", (B, 3, S, S)))
        _img_cache[(B, S)] = (cpu, cpu.cuda())
    return _img_cache[(B, S)]


def rows_of(x):
    """torch's gather: [B,3,S,S] -> [B*T, 768] in the kernels' layout."""
    return IM.patch_rows(x).reshape(-1, 768)


def guarded(M, dtype, dev):
    """an output buffer of M live rows with pad rows and a sentinel region behind them, all SENTINEL"""
    from devit_amd import ops
    return torch.full((ops.pad_rows(M) + TAIL_ROWS, 768), SENTINEL, dtype=dtype, device=dev)


def tail_ok(buf, M):
    return bool((buf[M:] == SENTINEL).all())


def boxes(S):
    """CutMix boxes (y0, y1, x0, x1): interior with both x edges inside an 8-pixel chunk, touching two edges (both ways), empty, the whole image"""
    return [(S // 4 + 1, S - 3, 5, S // 2 + 3), (0, S // 2, S // 2 + 1, S), (S // 2 - 1, S, 0, S // 3), (S // 2, S // 2, 3, S - 1), (0, S, 0, S)]


# ------------------------------------------------------------------------------------------ kernels, bit for bit
@pytest.mark.parametrize("S", KERNEL_SIZES)
@pytest.mark.parametrize("B", [1, 2, 3])
def test_im2row_bit_for_bit(dev, S, B):
    from devit_amd import ops
    from devit_amd._lib import call, ptr, stream_ptr
    cpu, img = images(B, S)
    M = B * (S // 16) ** 2
    want = rows_of(cpu)
    for dt in (BF16, F16):
        buf = guarded(M, dt, dev)
        call("devit_im2row_bf16", ptr(img), ptr(buf), B, 3, S, S, 16, int(dt == F16), stream_ptr())
        assert torch.equal(buf[:M].cpu(), want.to(dt)) and tail_ok(buf, M), (S, B, dt)
    buf = guarded(M, F32, dev)
    call("devit_im2row_f32_sized", ptr(img), ptr(buf), B, S, S, stream_ptr())
    assert torch.equal(buf[:M].cpu(), want) and tail_ok(buf, M), (S, B)
    pr = ops.patch_rows(img, dtypes=(BF16, F16))                      # the public wrapper: same bits, zero pad rows, the size on the result
    assert pr.shape == (B, 3, S, S) and pr.num_patches == (S // 16) ** 2
    assert torch.equal(pr.rows[:M].cpu(), want.to(BF16)) and torch.equal(pr.rows_f16[:M].cpu(), want.to(F16))
    assert not bool(pr.rows[M:].any()) and not bool(pr.rows_f16[M:].any())
    assert torch.equal(img.cpu(), cpu)


@pytest.mark.parametrize("S", KERNEL_SIZES)
@pytest.mark.parametrize("B", [1, 2, 3])
def test_batch_mixup_and_cutmix_bit_for_bit(dev, S, B):
    """devit_mix_im2row_bf16_sized: rows = bf16(lam * x + (1 - lam) * x[B-1-b]) with fp32 products and sum, f32(1 - lam) from a double
    subtraction (timm's batch mode); CutMix an exact copy inside the box."""
    from devit_amd._lib import call, ptr, stream_ptr
    cpu, img = images(B, S)
    M = B * (S // 16) ** 2
    flip = cpu.flip(0)

    def run(mode, lam, box):
        rb, rh = guarded(M, BF16, dev), guarded(M, F16, dev)
        call("devit_mix_im2row_bf16_sized", ptr(img), ptr(rb), ptr(rh), B, mode, float(lam), *box, S, S, stream_ptr())
        assert tail_ok(rb, M) and tail_ok(rh, M), (S, B, mode, box)
        return rb[:M].cpu(), rh[:M].cpu()
    for lam in (0.3, 0.75, 0.0, 1.0):
        want = cpu * torch.tensor(lam, dtype=F32) + flip * torch.tensor(1.0 - lam, dtype=torch.float64).to(F32)
        rb, rh = run(1, lam, (0, 0, 0, 0))
        assert torch.equal(rb, rows_of(want).to(BF16)) and torch.equal(rh, rows_of(want).to(F16)), (S, B, lam)
    for box in boxes(S):
        y0, y1, x0, x1 = box
        want = cpu.clone()
        want[:, :, y0:y1, x0:x1] = flip[:, :, y0:y1, x0:x1]
        rb, rh = run(2, 0.5, box)
        assert torch.equal(rb, rows_of(want).to(BF16)) and torch.equal(rh, rows_of(want).to(F16)), (S, B, box)
    rb, _ = run(0, 1.0, (0, 0, 0, 0))
    assert torch.equal(rb, rows_of(cpu).to(BF16))
    assert torch.equal(img.cpu(), cpu)


@pytest.mark.parametrize("S", KERNEL_SIZES)
@pytest.mark.parametrize("B", [1, 2, 3])
def test_table_kernel_bit_for_bit(dev, S, B):
    """devit_mix_im2row_table_sized: one (mode, lam, box) per sample, 1 - lam formed in fp32; bf16 rows, f16 rows and the fp32 img_out."""
    from devit_amd import ops
    from devit_amd._lib import call, ptr, stream_ptr
    cpu, img = images(B, S)
    T = (S // 16) ** 2
    M, n = B * T, B * 3 * S * S
    cut = lambda b: (2, float(np.float32(1 - (b[1] - b[0]) * (b[3] - b[2]) / (S * S)))) + b
    cases = [(0, 1.0, 0, 0, 0, 0), (1, 0.3, 0, 0, 0, 0), (1, 0.5000001, 0, 0, 0, 0), (1, 0.0, 0, 0, 0, 0)] + [cut(b) for b in boxes(S)]
    one = torch.tensor(1.0, dtype=F32)
    for s in range(0, len(cases), B):
        entries = [cases[(s + i) % len(cases)] for i in range(B)]
        table = ops.mix_table(entries, dev, img_size=S)
        want = torch.empty_like(cpu)
        for b, (mode, lam, y0, y1, x0, x1) in enumerate(entries):
            lam = torch.tensor(float(lam), dtype=F32)
            want[b] = cpu[b] * lam + cpu[B - 1 - b] * (one - lam) if mode == 1 else cpu[b]
            if mode == 2:
                want[b][:, y0:y1, x0:x1] = cpu[B - 1 - b][:, y0:y1, x0:x1]
        rb, rh = guarded(M, BF16, dev), guarded(M, F16, dev)
        im = torch.full((n + 1024,), SENTINEL, dtype=F32, device=dev)
        call("devit_mix_im2row_table_sized", ptr(img), ptr(rb), ptr(rh), ptr(im), ptr(table.dev), B, S, S, stream_ptr())
        assert tail_ok(rb, M) and tail_ok(rh, M) and bool((im[n:] == SENTINEL).all()), (S, B, entries)
        assert torch.equal(im[:n].view(B, 3, S, S).cpu(), want), (S, B, entries)
        assert torch.equal(rb[:M].cpu(), rows_of(want).to(BF16)) and torch.equal(rh[:M].cpu(), rows_of(want).to(F16)), (S, B, entries)
        assert torch.equal(ops.mix_patch_rows_table(img, table, f32_images=True).cpu(), want)
        assert torch.equal(ops.mix_patch_rows_table(img, table).rows[:M].cpu(), rows_of(want).to(BF16))
    with pytest.raises(ValueError):                      # a table whose boxes were checked against another image size
        ops.mix_patch_rows_table(img, ops.mix_table([(0, 1.0, 0, 0, 0, 0)] * B, dev))
    assert torch.equal(img.cpu(), cpu)


def test_sized_entry_points_at_224_give_the_bits_of_the_old_ones(dev):
    from devit_amd import ops
    from devit_amd._lib import call, ptr, stream_ptr
    B, M = 2, 2 * 196
    cpu, img = images(B, 224)
    for mode, lam, box in ((1, 0.3, (0, 0, 0, 0)), (2, 0.5, (37, 121, 13, 83)), (0, 1.0, (0, 0, 0, 0))):
        a, b = guarded(M, BF16, dev), guarded(M, BF16, dev)
        call("devit_mix_im2row_bf16", ptr(img), ptr(a), None, B, mode, lam, *box, stream_ptr())
        call("devit_mix_im2row_bf16_sized", ptr(img), ptr(b), None, B, mode, lam, *box, 224, 224, stream_ptr())
        assert torch.equal(a, b) and tail_ok(a, M)
    table = ops.mix_table([(1, 0.3, 0, 0, 0, 0), (2, 0.6, 10, 200, 3, 77)], dev)
    a, b = guarded(M, BF16, dev), guarded(M, BF16, dev)
    ia, ib = (torch.full((B * 3 * 224 * 224 + 1024,), SENTINEL, dtype=F32, device=dev) for _ in range(2))
    call("devit_mix_im2row_table", ptr(img), ptr(a), None, ptr(ia), ptr(table.dev), B, stream_ptr())
    call("devit_mix_im2row_table_sized", ptr(img), ptr(b), None, ptr(ib), ptr(table.dev), B, 224, 224, stream_ptr())
    assert torch.equal(a, b) and torch.equal(ia, ib) and tail_ok(a, M)
    a, b = guarded(M, F32, dev), guarded(M, F32, dev)
    call("devit_im2row_f32", ptr(img), ptr(a), B, stream_ptr())
    call("devit_im2row_f32_sized", ptr(img), ptr(b), B, 224, 224, stream_ptr())
    assert torch.equal(a, b) and torch.equal(a[:M].cpu(), rows_of(cpu)) and tail_ok(a, M)


def test_entry_points_refuse_other_sizes(dev):
    from devit_amd import ops
    from devit_amd._lib import DevitError, call, ptr, stream_ptr
    _, img = images(1, 32)
    buf = guarded(4, BF16, dev)
    for H, W in ((240, 240), (100, 100), (16, 16), (64, 32)):
        with pytest.raises(DevitError):
            call("devit_im2row_bf16", ptr(img), ptr(buf), 1, 3, H, W, 16, 0, stream_ptr())
        with pytest.raises(DevitError):
            call("devit_mix_im2row_bf16_sized", ptr(img), ptr(buf), None, 1, 0, 1.0, 0, 0, 0, 0, H, W, stream_ptr())
        with pytest.raises(DevitError):
            call("devit_im2row_f32_sized", ptr(img), ptr(buf), 1, H, W, stream_ptr())
    with pytest.raises(DevitError, match="outside 32x32"):           # the box is checked against H, W
        call("devit_mix_im2row_bf16_sized", ptr(img), ptr(buf), None, 1, 2, 0.5, 0, 33, 0, 8, 32, 32, stream_ptr())
    with pytest.raises(DevitError):
        ops.mix_patch_rows(img, 2, 0.5, (0, 8, 0, 40))
    assert tail_ok(buf, 0)


# ------------------------------------------------------------------------------------------ model
_model_cache = {}


def model_at(name, S, dev, **kw):
    """(HIP model on the device, its CPU state): built once per (name, size)."""
    import devit_amd
    key = (name, S, tuple(sorted(kw.items())))
    if key not in _model_cache:
        geom = O.GEOMETRY[name]
        st = IM.make_state(geom, C, "T" if geom["embed_dim"] == 768 else "S", S)
        m = devit_amd.create_model(name, num_classes=C, img_size=S, **kw)
        m.load_state_dict(st)
        _model_cache[key] = (m.to(dev), st)
    return _model_cache[key]


@pytest.mark.parametrize("name,S", [("dedeit", 32), ("dedeit", 112), ("dedeit", 208), ("devit", 48)])
def test_model_eval_vs_helper(dev, name, S):
    m, st = model_at(name, S, dev)
    geom = O.GEOMETRY[name]
    img = torch.from_numpy(det_array(f"imgsize/m{S}", (2, 3, S, S)))
    with torch.no_grad():
        ref = IM.forward(st, geom, img)
    N = (S // 16) ** 2 + m.num_tokens
    m.eval()
    try:
        m.precision = "f32"
        with torch.no_grad():
            out = m(img.to(dev))
            d = m(img.to(dev), output_qkv=True)
        e = rel(out, ref["output"])
        print(f"imgsize f32 {name} S={S}: logits rel {e:.3e}")
        assert chk(e, 1e-3, name=f"imgsize_f32_logits_{name}_{S}"), e
        assert torch.equal(out.argmax(1).cpu(), ref["output"].argmax(1))
        assert d["qkv"][5][0].shape == (2, geom["num_heads"], N, 64)
        assert chk(rel(d["qkv"][5][0], ref["qkv"][5][0]), 1e-3, name=f"imgsize_f32_q5_{name}_{S}")
    finally:
        m.precision = "bf16"
    with torch.no_grad():
        out = m(img.to(dev))
        d = m(img.to(dev), output_qkv=True)
    e = rel(out, ref["output"])
    print(f"imgsize bf16 {name} S={S}: logits rel {e:.3e}")
    ok = chk(e, 1.5e-2, name=f"imgsize_bf16_logits_{name}_{S}")
    eq = chk(rel(d["qkv"][5][0], ref["qkv"][5][0]), 2e-2, name=f"imgsize_bf16_q5_{name}_{S}")
    assert ok, f"logits rel-to-max err {e:.3e}"
    assert torch.equal(out.argmax(1).cpu(), ref["output"].argmax(1))
    assert eq


def test_lean_tail_is_bit_identical_at_6_tokens(dev):
    """S = 32: N = 6 tokens, fewer than one 16-row tile; the last block on its two token rows gives the full block's bits, as at 224."""
    from devit_amd import de_vit
    m, _ = model_at("dedeit", 32, dev)
    img = torch.from_numpy(det_array("imgsize/lean32", (3, 3, 32, 32))).to(dev)
    m.eval()
    with torch.no_grad():
        a = m(img)
        f = m(img, distill_token=True)
        with de_vit.lean_tail(m):
            b = m(img)
            d = m(img, distill_token=True)
    assert de_vit.LEAN_TAIL and torch.equal(a, b) and torch.equal(d["output"], a)
    assert torch.equal(d["last_tokens"][0], f["last_tokens"][0]) and torch.equal(d["last_tokens"][1], f["last_tokens"][1])


# ------------------------------------------------------------------------------------------ one DEKD step at S = 112
@pytest.fixture(scope="module")
def step112(dev):
    """One DEKD step at S = 112 (N = 51), B = 4, `dedeit` under DeiT-B with fixed DropPath scales: the helper's losses and gradients, once."""
    S, B = 112, 4
    s, st_s = model_at("dedeit", S, dev, drop_path_rate=0.1)
    t, st_t = model_at("deit_base_distilled_patch16_224", S, dev)
    t.eval()
    for p in t.parameters():
        p.requires_grad_(False)
    img = torch.from_numpy(det_array("imgsize/step112", (B, 3, S, S)))
    y1, y2 = det_labels("imgsize/sy1", B, C), det_labels("imgsize/sy2", B, C)
    oh = lambda y: torch.full((B, C), 0.1 / C).scatter_(1, torch.from_numpy(y)[:, None], 1 - 0.1 + 0.1 / C)
    soft = oh(y1) * 0.7 + oh(y2) * 0.3
    dps = IM.dp_scales_for("imgsize/step112", B)
    assert any(float(a.min()) == 0.0 or float(b.min()) == 0.0 for a, b in dps)         # some branch is dropped for some sample
    ref_st = {k: v.clone().requires_grad_(True) for k, v in st_s.items()}
    ref = IM.distill_step(ref_st, GS, st_t, GT, img, soft, dp_scales=dps)
    ref["loss"].backward()
    grads = {k: v.grad for k, v in ref_st.items()}
    return s, t, img, soft, dps, ref, grads


SLICES = [("head.weight", lambda g: g), ("blocks.5.attn.qkv.weight", lambda g: g[::48]), ("blocks.0.mlp.fc1.weight", lambda g: g[::64]),
          ("blocks.11.mlp.fc2.weight", lambda g: g[::16]), ("pos_embed", lambda g: g[0]), ("cls_token", lambda g: g),
          ("patch_embed.proj.weight", lambda g: g[::16].reshape(-1, 768)), ("norm.weight", lambda g: g)]


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_step_at_112_vs_helper(dev, step112, precision):
    from devit_amd import engine
    s, t, img, soft, dps, ref, grads = step112
    loss_bar, norm_bar, slice_bar, logit_bar = (1e-4, 1e-3, 1e-3, 1e-3) if precision == "f32" else (5e-4, 3e-3, 1.5e-2, 1.5e-2)
    try:
        s.precision = t.precision = precision
        s.train()
        for p in s.parameters():
            p.grad = None
        out = engine.distill_forward(s, t, img.to(dev), soft.to(dev), gama=(0.2, 0.1, 0.3), kind="hard", alpha=0.5, tau=1.0,
                                     dp_scales=[(a.to(dev).contiguous(), b.to(dev).contiguous()) for a, b in dps])
        fails = []
        for k in ("loss", "cls_loss", "q_loss", "k_loss", "v_loss"):
            e = abs(float(out[k].detach()) - float(ref[k].detach())) / abs(float(ref[k].detach()))
            print(f"imgsize step112 {precision} {k}: {float(out[k].detach()):.6f} vs {float(ref[k].detach()):.6f} rel {e:.3e}")
            if not chk(e, loss_bar, name=f"imgsize_step112_{precision}_{k}"):
                fails.append((k, e))
        if not chk(rel(out["teacher_logits"], ref["teacher"]["output"]), logit_bar, name=f"imgsize_step112_{precision}_teacher_logits"):
            fails.append("teacher_logits")
        out["loss"].backward()
        params = dict(s.named_parameters())
        names = list(params)
        gn = np.array([params[n].grad.norm().item() for n in names])
        rn = np.array([grads[n].norm().item() for n in names])
        if precision == "f32":
            worst = float(np.abs(gn - rn).max() / rn.max())
            if not chk(worst, norm_bar, name="imgsize_step112_f32_grad_norms"):
                fails.append(("grad norms", worst))
        else:
            chk(float((np.abs(gn - rn) / (rn + 1e-3 * rn.max())).max()), norm_bar, name="imgsize_step112_bf16_grad_norms")
            bad = np.abs(gn - rn) > norm_bar * rn + 3e-6 * rn.max()
            if bad.any():
                fails.append([(names[i], gn[i], rn[i]) for i in np.nonzero(bad)[0][:8]])
        for n, cut in SLICES:
            e = rel(cut(params[n].grad), cut(grads[n]))
            print(f"imgsize step112 {precision} grad {n}: rel {e:.3e}")
            if not chk(e, slice_bar, name=f"imgsize_step112_{precision}_g_{n}"):
                fails.append((n, e))
        assert not fails, fails
    finally:
        s.precision = t.precision = "bf16"
        for p in s.parameters():
            p.grad = None


# ------------------------------------------------------------------------------------------ plumbing
def test_a_model_refuses_a_batch_of_another_size(dev):
    from devit_amd import ops
    from devit_amd._lib import DevitError
    m, _ = model_at("dedeit", 32, dev)
    m.eval()
    img48 = images(2, 48)[1]
    with torch.no_grad():
        for prec in ("bf16", "f32"):
            try:
                m.precision = prec
                with pytest.raises(DevitError, match=r"32 x 32.*48 x 48"):
                    m(img48)
            finally:
                m.precision = "bf16"
        with pytest.raises(DevitError, match=r"32 x 32.*48 x 48"):
            m(ops.patch_rows(img48))
        m112, _ = model_at("dedeit", 112, dev)
        with pytest.raises(DevitError, match=r"112 x 112.*32 x 32"):
            m112(ops.patch_rows(images(2, 32)[1]))
        assert m(ops.patch_rows(images(2, 32)[1])).shape == (2, C)


@pytest.mark.parametrize("mode", ["elem", "batch"])
def test_mixup_at_64_feeds_the_model_the_rows_of_its_draw(dev, mode):
    """Mixup(mode=...)(x, y) on 64 x 64 images (--mixup-mode elem / batch at --input-size 64): the rows are those of the torch mix of its
    own draw, with the boxes drawn on 64 x 64."""
    from devit_amd import ops
    from distill_sub import Mixup
    S, B = 64, 6
    cpu = torch.from_numpy(det_array("imgsize/mix64", (B, 3, S, S)))
    y = torch.from_numpy(det_labels("imgsize/mixy", B, 10)).to(dev)
    mx = Mixup(0.8, 1.0, 1.0, 0.5, 0.1, 10, mode=mode, img_size=S)
    one = torch.tensor(1.0, dtype=F32)
    for seed in (1, 2, 3, 4):
        np.random.seed(seed)
        entries = [tuple(e)[:6] for e in mx.draw_table(B, S, S).tolist()] if mode == "elem" else None
        if mode == "batch":
            md, lam, box = mx.draw(S, S)
        np.random.seed(seed)
        pr, targets = mx(cpu.to(dev), y)
        assert isinstance(pr, ops.PatchRows) and pr.shape == (B, 3, S, S) and targets.shape == (B, 10)
        want = torch.empty_like(cpu)
        for b in range(B):
            if mode == "elem":
                m_, l_, y0, y1, x0, x1 = entries[b]
                l_, oml = torch.tensor(float(l_), dtype=F32), None
                oml = one - l_
            else:
                m_, (y0, y1, x0, x1) = md, box
                l_, oml = torch.tensor(lam, dtype=F32), torch.tensor(1.0 - lam, dtype=torch.float64).to(F32)
            want[b] = cpu[b] * l_ + cpu[B - 1 - b] * oml if m_ == 1 else cpu[b]
            if m_ == 2:
                assert 0 <= y0 <= y1 <= S and 0 <= x0 <= x1 <= S
                want[b][:, y0:y1, x0:x1] = cpu[B - 1 - b][:, y0:y1, x0:x1]
        assert torch.equal(pr.rows[: B * 16].cpu(), rows_of(want).to(BF16)), (mode, seed)
    m, _ = model_at("dedeit", 64, dev)                  # ... and a 64-pixel model reads them
    m.eval()
    with torch.no_grad():
        assert torch.equal(m(pr), m(ops.patch_rows(want.to(dev))))
    if mode == "elem":                                  # a Mixup set up for one size refuses a batch of another in the table modes
        with pytest.raises(NotImplementedError, match="64 x 64"):
            mx(torch.zeros(2, 3, 112, 112, device=dev), y[:2])


def _run_cli(script, argv, tmp_path, limit=240):
    """One child-process run of a CLI under its own time limit -> its stdout."""
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.join(ROOT, script)] + argv + ["--output_dir", str(tmp_path)]
    r = subprocess.run(cmd, cwd=str(tmp_path), env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-3000:])
    return r.stdout


def test_distill_sub_cli_at_64(dev, tmp_path):
    out = _run_cli("distill_sub.py", ["--synthetic", "2", "--batch-size", "8", "--input-size", "64", "--epochs", "1", "--warmup-epochs", "0",
                                      "--model", "dedeit", "--teacher-model", "deit_base_distilled_patch16_224"], tmp_path)
    m = re.search(r"\[Train\] Loss: ([-+0-9.einfa]+)", out)
    assert m and np.isfinite(float(m.group(1))), out[-2000:]
    ck = torch.load(next(tmp_path.rglob("checkpoint_temp.pth")), map_location="cpu", weights_only=False)
    assert tuple(ck["model"]["pos_embed"].shape) == (1, 18, 384) and ck["args"].input_size == 64


def test_ensemble_cli_eval_at_64(dev, tmp_path):
    out = _run_cli("ensemble.py", ["--synthetic", "8", "--batch-size", "8", "--input-size", "64", "--eval", "--model", "dedeit",
                                   "--teacher-model", "deit_base_distilled_patch16_224", "--sub_classes", "5", "5"], tmp_path)
    m = re.search(r"'loss': ([-+0-9.einfa]+)", out)
    assert m and np.isfinite(float(m.group(1))), out[-2000:]
