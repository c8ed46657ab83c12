"""Per-sample Mixup / CutMix on the device (timm Mixup mode='elem' / 'pair'): devit_mix_im2row_table and devit_mix_targets_table bit for bit
against the fp32 statement written out in torch below, against the batch-mode kernels where the two must agree, through a model, and through
two CLIs.  The statement (per sample b, partner B-1-b, every operand an fp32 tensor, every operation rounded on its own):
    mode 1: x[b] * lam + x[B-1-b] * (1f - lam)        mode 2: x[b] with [y0,y1) x [x0,x1) copied from x[B-1-b]        mode 0: x[b]
rounded ONCE to the 16-bit type of the rows.  Images are 224 x 224 (the patchify is built for that); B = 6 and 2 are several workgroups per
sample and the smallest even batch."""
import argparse
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
IMG = 3 * 224 * 224


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from devit_amd import _lib
    _lib.require_device(torch.zeros(1, device="cuda"))
    return torch.device("cuda")


def cut(y0, y1, x0, x1):
    return (2, float(np.float32(1 - (y1 - y0) * (x1 - x0) / (224 * 224))), y0, y1, x0, x1)


# every case the kernel tells apart; a table of B entries is a window of this list, and the windows of one B cover it
CASES = [
    (0, 1.0, 0, 0, 0, 0),
    (1, 0.3, 0, 0, 0, 0),
    (1, 0.75, 0, 0, 0, 0),
    (1, 0.0, 0, 0, 0, 0),
    cut(37, 121, 13, 83),           # interior; x0 and x1 are no multiples of 8: both edges fall inside an 8-element chunk
    cut(0, 224, 0, 224),            # the whole image
    (2, 1.0, 50, 50, 10, 100),      # empty (y0 == y1)
    cut(0, 100, 150, 224),          # touches 0 on y and 224 on x
    cut(120, 224, 0, 75),           # touches 224 on y and 0 on x
    cut(5, 6, 17, 18),              # one pixel
    (1, 1.0, 0, 0, 0, 0),
    (1, 0.5000001, 0, 0, 0, 0),
]


def tables_for(B):
    return [[CASES[(s + i) % len(CASES)] for i in range(B)] for s in range(0, len(CASES), B)]


_img_cache = {}


def images(B):
    """(cpu, device) copies of the deterministic batch; computed once per B, never written."""
    if B not in _img_cache:
        from oracle.detgen import det_array
        cpu = torch.from_numpy(det_array("mixmodes/img", (B, 3, 224, 224)))
        _img_cache[B] = (cpu, cpu.cuda())
    return _img_cache[B]


def torch_mix(x, entries):
    """The statement of the module docstring on fp32 CPU tensors; x is not written."""
    B = x.shape[0]
    out = torch.empty_like(x)
    one = torch.tensor(1.0, dtype=F32)
    for b, (mode, lam, y0, y1, x0, x1) in enumerate(entries):
        mode, (y0, y1, x0, x1) = int(mode), (int(v) for v in (y0, y1, x0, x1))
        lam = torch.tensor(float(lam), dtype=F32)
        if mode == 1:
            out[b] = x[b] * lam + x[B - 1 - b] * (one - lam)
        else:
            out[b] = x[b]
            if mode == 2:
                out[b][:, y0:y1, x0:x1] = x[B - 1 - b][:, y0:y1, x0:x1]
    return out


def torch_targets(y, entries, Cn, smoothing):
    B = y.shape[0]
    off = torch.tensor(smoothing / Cn, dtype=torch.float64).to(F32)
    on = torch.tensor(1.0 - smoothing + smoothing / Cn, dtype=torch.float64).to(F32)
    hot = torch.nn.functional.one_hot(y, Cn).bool()
    t = torch.where(hot, on, off)
    lam = torch.tensor([float(e[1]) for e in entries], dtype=F32).view(B, 1)
    return t * lam + t.flip(0) * (torch.tensor(1.0, dtype=F32) - lam)


def unrow(rows, B):
    """patch rows [B*196, 768] -> image layout [B, 3, 224, 224]."""
    return rows[: B * 196].view(B, 14, 14, 3, 16, 16).permute(0, 3, 1, 4, 2, 5).reshape(B, 3, 224, 224)


SENTINEL = 7.0
TAIL_ROWS = 8


def launch(img, table, want_bf16, want_f16, want_f32):
    """devit_mix_im2row_table into buffers with a sentinel behind everything the kernel may write -> (bf16 rows, f16 rows, images, tails ok)"""
    from devit_amd import ops
    from devit_amd._lib import call, ptr, stream_ptr
    B, M = img.shape[0], img.shape[0] * 196
    mk = lambda dt: torch.full((ops.pad_rows(M) + TAIL_ROWS, 768), SENTINEL, dtype=dt, device=img.device)
    rb, rh = (mk(BF16) if want_bf16 else None), (mk(F16) if want_f16 else None)
    im = torch.full((B * IMG + 1024,), SENTINEL, dtype=F32, device=img.device) if want_f32 else None
    call("devit_mix_im2row_table", ptr(img), ptr(rb), ptr(rh), ptr(im), ptr(table.dev), B, stream_ptr())
    tails = all(bool((t[M:] == SENTINEL).all()) for t in (rb, rh) if t is not None) and (im is None or bool((im[B * IMG:] == SENTINEL).all()))
    return rb, rh, (im[: B * IMG].view(B, 3, 224, 224) if want_f32 else None), tails


@pytest.mark.parametrize("B", [6, 2])
def test_rows_and_images_bit_for_bit(dev, B):
    from devit_amd import ops
    cpu, img = images(B)
    seen = set()
    for entries in tables_for(B):
        seen |= set(entries)
        table = ops.mix_table(entries, dev)
        assert table.host.tobytes() == ops.mix_entries(entries).tobytes() and table.dev.cpu().numpy().tobytes() == table.host.tobytes()
        want = torch_mix(cpu, entries)
        want_b, want_h = want.to(BF16), want.to(F16)
        for outs in ((1, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1)):
            rb, rh, im, tails = launch(img, table, *outs)
            assert tails, (entries, outs)
            if rb is not None:
                assert torch.equal(unrow(rb, B).cpu(), want_b), (entries, outs)
            if rh is not None:
                assert torch.equal(unrow(rh, B).cpu(), want_h), (entries, outs)
            if im is not None:
                assert torch.equal(im.cpu(), want), (entries, outs)
        assert torch.equal(img.cpu(), cpu)                      # the input is only read
        # the public wrappers: the same bits, zero pad rows
        pr = ops.mix_patch_rows_table(img, table, dtypes=(BF16, F16))
        assert torch.equal(unrow(pr.rows, B).cpu(), want_b) and torch.equal(unrow(pr.rows_f16, B).cpu(), want_h)
        assert not bool(pr.rows[B * 196:].any()) and not bool(pr.rows_f16[B * 196:].any())
        assert ops.mix_patch_rows_table(img, table).rows_f16 is None
        assert torch.equal(ops.mix_patch_rows_table(img, table, f32_images=True).cpu(), want)
    assert seen == set(CASES)


@pytest.mark.parametrize("B", [6, 2])
@pytest.mark.parametrize("Cn", [25, 7])
@pytest.mark.parametrize("smoothing", [0.1, 0.0])
def test_targets_bit_for_bit(dev, B, Cn, smoothing):
    from oracle.detgen import det_labels
    from devit_amd import ops
    y = torch.from_numpy(det_labels("mixmodes/y", B, Cn))
    for entries in tables_for(B):
        table = ops.mix_table(entries, dev)
        got = ops.mix_targets_table(y.to(dev), Cn, table, smoothing).cpu()
        assert got.shape == (B, Cn) and torch.equal(got, torch_targets(y, entries, Cn, smoothing)), entries
        assert float((got.sum(1) - 1).abs().max()) < 1e-6


def test_agrees_with_the_batch_kernels(dev):
    """Where the two families must give the same bits: lam 0.75 (1 - lam is the same in fp32 and in double), and CutMix with one box."""
    from oracle.detgen import det_labels
    from devit_amd import ops
    B, Cn = 6, 25
    _, img = images(B)
    y = torch.from_numpy(det_labels("mixmodes/y", B, Cn)).to(dev)
    both = (BF16, F16)
    t = ops.mix_table([(1, 0.75, 0, 0, 0, 0)] * B, dev)
    a, b = ops.mix_patch_rows_table(img, t, dtypes=both), ops.mix_patch_rows(img, 1, 0.75, dtypes=both)
    assert torch.equal(a.rows, b.rows) and torch.equal(a.rows_f16, b.rows_f16)
    assert torch.equal(ops.mix_targets_table(y, Cn, t, 0.1), ops.mix_targets(y, Cn, 0.75, 0.1))
    box = (37, 121, 13, 83)
    t = ops.mix_table([cut(*box)] * B, dev)
    a, b = ops.mix_patch_rows_table(img, t, dtypes=both), ops.mix_patch_rows(img, 2, 1.0, box, dtypes=both)
    assert torch.equal(a.rows, b.rows) and torch.equal(a.rows_f16, b.rows_f16)
    t = ops.mix_table([(0, 1.0, 0, 0, 0, 0)] * B, dev)
    assert torch.equal(ops.mix_patch_rows_table(img, t).rows, ops.patch_rows(img).rows)


def test_refusals(dev):
    from devit_amd import ops
    from devit_amd._lib import DevitError, call, ptr, stream_ptr
    B = 2
    _, img = images(B)
    table = ops.mix_table([(1, 0.5, 0, 0, 0, 0)] * B, dev)
    with pytest.raises(DevitError, match="img_out is img"):
        call("devit_mix_im2row_table", ptr(img), None, None, ptr(img), ptr(table.dev), B, stream_ptr())
    with pytest.raises(DevitError):
        call("devit_mix_im2row_table", ptr(img), None, None, None, ptr(table.dev), B, stream_ptr())         # no output at all
    rows = ops.rows_alloc(B * 196, 768, BF16, dev)
    with pytest.raises(DevitError):
        call("devit_mix_im2row_table", ptr(img), ptr(rows), None, None, None, B, stream_ptr())              # no table
    with pytest.raises(ValueError):
        ops.mix_patch_rows_table(img, ops.mix_table([(1, 0.5, 0, 0, 0, 0)] * 4, dev))                         # a table of another batch
    assert torch.equal(img.cpu(), images(B)[0])


def test_uploads_back_to_back_each_arrive(dev):
    """mix_table never waits for the stream: tables uploaded back to back with nothing synchronising in between, fewer of them than the
    pinned ring has slots (beyond that the ring relies on the stream having caught up, as its docstring says), each arrive as written; and
    'cuda' and 'cuda:N' share one ring."""
    from devit_amd import ops
    n = ops.MIX_RING_SLOTS - 56
    many = [ops.mix_table([(1, (k % 100) / 100.0, 0, 0, 0, 0)] * 4, dev if k % 2 else torch.device("cuda", torch.cuda.current_device()))
            for k in range(n)]
    assert len(ops._mix_ring) == 1
    for k, t in enumerate(many):
        assert t.dev.cpu().numpy().tobytes() == t.host.tobytes() and t.host["lam"][0] == np.float32((k % 100) / 100.0)


def _mixup(mode, **kw):
    from distill_sub import Mixup
    return Mixup(0.8, 1.0, 1.0, 0.5, 0.1, 10, mode=mode, **kw)


@pytest.mark.parametrize("mode,kw", [("elem", {}), ("pair", {"cutmix_minmax": (0.2, 0.6)})])
def test_through_the_model(dev, mode, kw):
    """Mixup(mode=...)(x, y) feeds a model the rows of exactly the mix its draw_table describes: logits equal, bit for bit, those of the same
    model on ops.patch_rows of the torch mix of the fp32 images."""
    import devit_amd
    from oracle.detgen import det_labels
    from devit_amd import ops
    B = 4
    cpu, img = images(6)
    cpu, img = cpu[:B], img[:B].contiguous()
    y = torch.from_numpy(det_labels("mixmodes/y", B, 10))
    torch.manual_seed(4)
    m = devit_amd.create_model("dedeit", depth=2, num_classes=10).to(dev).eval()
    mix = _mixup(mode, **kw)
    np.random.seed(11)
    tab = mix.draw_table(B)
    assert (tab["mode"] != 0).any()
    entries = [tuple(e)[:6] for e in tab.tolist()]
    np.random.seed(11)
    rows, targets = mix(img, y.to(dev))
    assert isinstance(rows, ops.PatchRows) and torch.equal(img.cpu(), cpu)
    want = torch_mix(cpu, entries)
    assert torch.equal(unrow(rows.rows, B).cpu(), want.to(BF16))
    assert torch.equal(targets.cpu(), torch_targets(y, entries, 10, 0.1))
    with torch.no_grad():
        assert torch.equal(m(rows), m(ops.patch_rows(want.to(dev))))


def test_through_an_f32_model(dev):
    """With an "f32" model among the readers the mixed batch is the kernel's fp32-image output: bit-equal to the torch mix, and so are the logits."""
    import devit_amd
    from oracle.detgen import det_labels
    B = 4
    cpu, img = images(6)
    cpu, img = cpu[:B], img[:B].contiguous()
    y = torch.from_numpy(det_labels("mixmodes/y", B, 10))
    torch.manual_seed(4)
    m = devit_amd.create_model("dedeit", depth=1, num_classes=10).to(dev).eval()
    m.precision = "f32"
    mix = _mixup("elem")
    mix.set_precisions("f32", "bf16")
    np.random.seed(5)
    entries = [tuple(e)[:6] for e in mix.draw_table(B).tolist()]
    np.random.seed(5)
    mixed, targets = mix(img, y.to(dev))
    want = torch_mix(cpu, entries)
    assert torch.is_tensor(mixed) and mixed.dtype == F32 and mixed.data_ptr() != img.data_ptr()
    assert torch.equal(mixed.cpu(), want) and torch.equal(img.cpu(), cpu)
    assert torch.equal(targets.cpu(), torch_targets(y, entries, 10, 0.1))
    with torch.no_grad():
        assert torch.equal(m(mixed), m(want.to(dev)))


def test_table_modes_need_224(dev):
    with pytest.raises(NotImplementedError):
        _mixup("elem")(torch.zeros(2, 3, 112, 112, device=dev), torch.zeros(2, dtype=torch.long, device=dev))


# ------------------------------------------------------------------------------------------ the flags, end to end
def _run_cli(mod, tmp_path, extra):
    parser = argparse.ArgumentParser(parents=[mod.get_args_parser()], conflict_handler="resolve")
    args = parser.parse_args(["--synthetic", "2", "--batch-size", "4", "--epochs", "1", "--warmup-epochs", "0", "--model", "dedeit",
                              "--teacher-model", "deit_base_distilled_patch16_224", "--dataset", "cifar100", "--num_division", "4",
                              "--output_dir", str(tmp_path)] + extra)
    seen = []
    from devit_amd import ops
    real = ops.mix_patch_rows_table

    def spy(img, table, **kw):
        seen.append(table.host.copy())
        return real(img, table, **kw)
    ops.mix_patch_rows_table = spy
    try:
        mod.main(args)
    finally:
        ops.mix_patch_rows_table = real
    line = json.loads(open(os.path.join(args.output_dir, "sub-dataset0", "log.txt")).read().splitlines()[-1])
    assert np.isfinite(line["train_loss"])
    assert len(seen) == 2 and all(t.shape == (4,) for t in seen)        # every step went through the table kernel
    return seen


def test_distill_sub_cli_pair_minmax(dev, tmp_path):
    import distill_sub
    for t in _run_cli(distill_sub, tmp_path, ["--mixup-mode", "pair", "--cutmix-minmax", "0.2", "0.6"]):
        assert t[0] == t[3] and t[1] == t[2]
        for e in t[t["mode"] == 2]:
            assert int(224 * 0.2) <= e["y1"] - e["y0"] < int(224 * 0.6) and int(224 * 0.2) <= e["x1"] - e["x0"] < int(224 * 0.6)


def test_train_subdata_cli_elem(dev, tmp_path):
    import train_subdata
    _run_cli(train_subdata, tmp_path, ["--mixup-mode", "elem"])
