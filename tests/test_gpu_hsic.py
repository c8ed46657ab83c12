"""The ranking kernels of the shrink stage (csrc/hsic.hip) against a float64 CPU evaluation of the repository's own
restatement (shrink._hsic / _gauss_mix on .double() tensors), the golden ranks, a real forward's activations, the policy
search and the shrink.py -> distill_sub.py chain.

Bar for rel, red and the final scores: |score - ref| <= 2e-5 * max|ref| on identical inputs rounded to the type fed to the
kernel (the project's fp32-kernel bar; the fp32 torch statement sits at 1e-7 .. 2.6e-7 of it on the
CPU); act is a plain sum and is held to 1e-6 relative.  Every measured deviation goes through conftest.chk under a name that starts
with "hsic", so it lands in the session's parity margins; profiles/hsic_parity.json is the committed copy of those rows."""
import argparse
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, chk

pytestmark = pytest.mark.gpu

BAR, ACT_BAR = 2e-5, 1e-6


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda")


def _dev(case, what, got, ref, bar=BAR):
    """max |got - ref| / max |ref|, recorded; True when inside the bar"""
    got, ref = got.detach().double().cpu(), ref.double()
    d = float((got - ref).abs().max() / ref.abs().max())
    print(f"{case} {what}: {d:.3e} (bar {bar:.0e})")
    return chk(d, bar, name=f"hsic {case} {what}")


def _no_constant_nonzero_columns(x):
    """x [B, ..., features]: no feature column (one unit at one token) is constant over the batch unless it is all zero"""
    same = (x == x[:1]).all(0)
    return not bool((same & (x[0] != 0)).any())


def _separate_constant_columns(x):
    """Inputs are CHOSEN without constant non-zero columns (16-bit rounding makes two samples of a column collide now and
    then at B = 2): sample 0 of such a column moves to a neighbouring representable value."""
    for _ in range(4):
        same = (x == x[:1]).all(0) & (x[0] != 0)
        if not bool(same.any()):
            break
        x[0] = torch.where(same, x[0] * 1.0078125, x[0])
    return x


_CASES = {}


def _neuron_case(B, N, units, dtype):
    """post-GELU-like activations with one all-zero (masked) unit, the logits, and the float64 reference -- made once"""
    key = ("n", B, N, units, dtype)
    if key not in _CASES:
        from devit_amd import shrink
        g = torch.Generator().manual_seed(1000 + B + units)
        x = torch.nn.functional.gelu(torch.randn((B, N, units), generator=g) * 1.5).to(dtype)
        x[:, :, 5] = 0
        x = _separate_constant_columns(x)
        logits = torch.randn((B, 25), generator=g) * 2
        xd, prob = x.double(), torch.softmax(logits.double(), -1)
        rel = shrink._hsic(xd.permute(2, 0, 1), prob, 'linear', True)
        act = xd.abs().sum((0, 1))
        mm = lambda v: (v - v.min()) / (v.max() - v.min())
        _CASES[key] = (x, logits, rel, act, 0.1 * mm(rel) + 0.9 * mm(act))
    return _CASES[key]


def _head_reference(hd_out, prob):
    from devit_amd import shrink
    Hh = hd_out.double().mean(-1).permute(2, 0, 1)
    H = Hh.shape[0]
    rel = shrink._hsic(Hh, prob, 'linear', True)
    red = torch.stack([sum(shrink._hsic(Hh[a], Hh[b], 'rbf', False) for b in range(H) if b != a) / (H - 1) for a in range(H)])
    return rel, red, rel - 0.1 * red


NEURON_SHAPES = [(2, 198, 128), (37, 198, 192), (130, 198, 64), (256, 198, 64)]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("B,N,units", NEURON_SHAPES)
def test_neuron_scores_against_float64(B, N, units, dtype):
    dev = _need_gpu()
    from devit_amd import shrink
    x, logits, rel_ref, act_ref, score_ref = _neuron_case(B, N, units, dtype)
    assert _no_constant_nonzero_columns(x) and bool((x[:, :, 5] == 0).all())
    case = f"neurons B{B} N{N} u{units} {str(dtype)[6:]}"
    xg = x.to(dev)
    W = shrink.hsic_target(logits.to(dev), softmax=True)
    rel, act, _ = shrink.hsic_unit_scores(xg, W, 1, want_act=True)
    ok = _dev(case, "rel", rel, rel_ref)
    a, r = act.double().cpu(), act_ref
    act_dev = float(((a - r).abs() / r.clamp_min(1e-300)).max())
    print(f"{case} act: {act_dev:.3e} (bar {ACT_BAR:.0e})")
    ok &= chk(act_dev, ACT_BAR, name=f"hsic {case} act")
    assert float(act[5]) == 0.0
    score = shrink.neuron_scores(xg, torch.softmax(logits, -1).to(dev))          # the public entry: probabilities in
    ok &= _dev(case, "score", score, score_ref)
    assert ok


def test_neuron_scores_on_a_strided_view():
    """the forward's neuron_output is a [:M] view of a padded, wider row buffer: rows are read in place through the strides"""
    dev = _need_gpu()
    from devit_amd import shrink
    B, N, units = 37, 198, 192
    x, logits, rel_ref, act_ref, _ = _neuron_case(B, N, units, torch.bfloat16)
    buf = torch.full((B * N + 58, units + 64), 7.0, dtype=torch.bfloat16, device=dev)       # junk around the view
    view = buf[:B * N].view(B, N, units + 64)[:, :, :units]
    view.copy_(x.to(dev))
    assert not view.is_contiguous() and view.stride(2) == 1 and view.stride(1) == units + 64
    W = shrink.hsic_target(logits.to(dev), softmax=True)
    rel, act, _ = shrink.hsic_unit_scores(view, W, 1, want_act=True)
    rel_c, act_c, _ = shrink.hsic_unit_scores(x.to(dev), W, 1, want_act=True)
    assert torch.equal(rel, rel_c) and torch.equal(act, act_c)          # same values, same order of operations
    assert _dev("neurons strided view B37 bf16", "rel", rel, rel_ref)


HEAD_SHAPES = [(6, 20, 4, 8), (37, 198, 6, 64), (130, 198, 12, 64), (2, 198, 6, 64)]


@pytest.mark.parametrize("B,N,H,hd", HEAD_SHAPES)
def test_head_scores_against_float64(B, N, H, hd):
    dev = _need_gpu()
    from devit_amd import shrink
    g = torch.Generator().manual_seed(2000 + B + H)
    x = (torch.randn((B, N, H, hd), generator=g) * 0.5 + torch.randn((B, N, H, 1), generator=g) * 0.3).to(torch.bfloat16)
    if B == 37:
        x[:, :, 2] = 0                                   # a masked head
    logits = torch.randn((B, 25), generator=g) * 2
    feat = x.double().mean(-1)
    assert _no_constant_nonzero_columns(feat)
    prob = torch.softmax(logits.double(), -1)
    rel_ref, red_ref, score_ref = _head_reference(x, prob)
    case = f"heads B{B} N{N} H{H} hd{hd} bf16"
    xg = x.to(dev)
    W = shrink.hsic_target(logits.to(dev), softmax=True)
    rel, _, kmix = shrink.hsic_unit_scores(xg.view(B, N, H * hd), W, hd, want_kmix=True)
    ok = _dev(case, "rel", rel, rel_ref)
    from devit_amd._lib import call, ptr, stream_ptr
    red = torch.empty((H,), dtype=torch.float32, device=dev)
    call("devit_hsic_head_pairs", ptr(kmix), H, B, ptr(red), stream_ptr())
    ok &= _dev(case, "red", red, red_ref)
    ok &= _dev(case, "score", shrink.head_scores(xg, torch.softmax(logits, -1).to(dev)), score_ref)
    # the kernel matrix itself (stored minus one): symmetric, zero diagonal, the mix of the five Gaussians
    assert torch.equal(kmix, kmix.transpose(1, 2)) and bool((torch.diagonal(kmix, dim1=1, dim2=2) == 0).all())
    ok &= _dev(case, "Kmix - 1", kmix, shrink._gauss_mix(x.double().mean(-1).permute(2, 0, 1)) - 1)
    assert ok


def test_f16_elements():
    dev = _need_gpu()
    from devit_amd import shrink
    x, logits, _, _, _ = _neuron_case(37, 198, 192, torch.float32)
    x16 = _separate_constant_columns(x.to(torch.float16))
    assert _no_constant_nonzero_columns(x16)
    prob = torch.softmax(logits.double(), -1)
    rel_ref = shrink._hsic(x16.double().permute(2, 0, 1), prob, 'linear', True)
    rel, _, _ = shrink.hsic_unit_scores(x16.to(dev), shrink.hsic_target(logits.to(dev), softmax=True), 1)
    assert _dev("neurons B37 N198 u192 float16", "rel", rel, rel_ref)


def test_golden_ranks_on_the_device():
    """tests/golden/imp_rank.npz (the reference's own ranks on synthetic activations) fed as f32: the argsort of the device
    scores is the golden rank exactly (smallest neighbouring gap: 1.2e-4 of a range of about 1 for the neurons, 2.9e-3 for
    the heads)."""
    dev = _need_gpu()
    from devit_amd import shrink
    g = dict(np.load(os.path.join(GOLDEN, "imp_rank.npz")))
    prob = torch.softmax(torch.from_numpy(g["logits"]), -1).to(dev)
    for i in range(2):
        ns = shrink.neuron_scores(torch.from_numpy(g[f"n{i}"]).to(dev), prob)
        hs = shrink.head_scores(torch.from_numpy(g[f"h{i}"]).to(dev), prob)
        assert np.array_equal(np.argsort(ns.cpu().numpy()), g["neuron_rank"][i])
        assert np.array_equal(np.argsort(hs.cpu().numpy()), g["head_rank"][i])


def test_too_large_a_batch_is_refused():
    dev = _need_gpu()
    from devit_amd import shrink
    from devit_amd._lib import DevitError
    with pytest.raises(DevitError, match="outside 2..256"):
        shrink.hsic_unit_scores(torch.zeros((257, 4, 64), dtype=torch.bfloat16, device=dev), torch.zeros((257, 257), device=dev), 1)


@pytest.fixture(scope="module")
def dedeit():
    dev = _need_gpu()
    import devit_amd
    torch.manual_seed(4)
    m = devit_amd.create_model("dedeit", num_classes=25).to(dev).eval()
    g = torch.Generator().manual_seed(9)
    return m, torch.randn((8, 3, 224, 224), generator=g).to(dev)


def test_scores_of_a_real_forward(dedeit):
    """dedeit at bs 8, blocks 0 and 11: the views the forward left on the modules (bf16, hidden 1536, their real strides)
    against float64 on CPU copies.  A real forward does produce feature columns that are constant and non-zero over the batch
    (the class token's row enters block 0 identical for every image): for units with such a column the reference value is
    cancellation noise and the float64 reference is the translation-invariant statement (_hsic on centred targets without
    the per-column shift); for every other unit the two float64 statements are shown to be the same number."""
    dev = _need_gpu()
    from devit_amd import shrink
    m, img = dedeit
    with torch.no_grad():
        out = m(img)
    out = (out[0] + out[1]) / 2 if isinstance(out, tuple) else out
    W = shrink.hsic_target(out, softmax=True)
    prob = torch.softmax(out.double().cpu(), -1)
    yc = prob - prob.mean(0, keepdim=True)
    ok = True
    for i in (0, 11):
        no, ho = m.blocks[i].mlp.neuron_output, m.blocks[i].attn.head_output
        assert no.shape == (8, 198, 1536) and ho.shape == (8, 198, 6, 64) and no.dtype == torch.bfloat16
        xd = no.double().cpu()
        ref = shrink._hsic(xd.permute(2, 0, 1), yc, 'linear', False)
        clean = ~((xd == xd[:1]).all(0) & (xd[0] != 0)).any(0)                     # units without a constant non-zero column
        shifted = shrink._hsic(xd.permute(2, 0, 1)[clean], prob, 'linear', True)
        assert int(clean.sum()) > 0 and float((shifted - ref[clean]).abs().max()) <= 1e-6 * float(ref.abs().max())
        rel, act, _ = shrink.hsic_unit_scores(no, W, 1, want_act=True)
        ok &= _dev(f"dedeit bs8 block {i} neurons", "rel", rel, ref)
        a, r = act.double().cpu(), xd.abs().sum((0, 1))
        ok &= chk(float(((a - r).abs() / r.clamp_min(1e-300)).max()), ACT_BAR)
        hd_ = ho.double().cpu()
        Hh = hd_.mean(-1).permute(2, 0, 1)
        rel_ref = shrink._hsic(Hh, yc, 'linear', False)
        red_ref = torch.stack([sum(shrink._hsic(Hh[a_], Hh[b_], 'rbf', False) for b_ in range(6) if b_ != a_) / 5 for a_ in range(6)])
        ok &= _dev(f"dedeit bs8 block {i} heads", "score", shrink._head_scores_device(ho, W), rel_ref - 0.1 * red_ref)
    assert ok


def test_rank_units_sums_batches(dedeit):
    dev = _need_gpu()
    from devit_amd import shrink
    m, img = dedeit
    g = torch.Generator().manual_seed(10)
    other = torch.randn((8, 3, 224, 224), generator=g).to(dev)
    lab = torch.zeros(8, dtype=torch.long, device=dev)
    n1, h1 = shrink.rank_units(m, [(img, lab), (other, lab)], dev)
    n1b, _ = shrink.rank_units(m, [(img, lab)], dev, batches=2)                  # a loader shorter than `batches` is used up
    n2, h2 = shrink.rank_units(m, [(img, lab), (other, lab)], dev, batches=2)
    assert all(np.array_equal(a, b) for a, b in zip(n1, n1b)) and len(n2) == len(h2) == 12
    assert any(not np.array_equal(a, b) for a, b in zip(n1, n2))                 # the second batch entered
    assert sorted(n2[3].tolist()) == list(range(1536)) and sorted(h2[3].tolist()) == list(range(6))
    assert not m.training


def test_search_policy(dedeit):
    dev = _need_gpu()
    from devit_amd import flops, shrink
    m, img = dedeit
    lab = torch.arange(8, device=dev) % 25
    with torch.no_grad():
        before = m(img)
        before = tuple(t.clone() for t in before) if isinstance(before, tuple) else before.clone()
    nr, hr = shrink.rank_units(m, [(img, lab)], dev)
    geo = shrink.model_geometry(m)
    assert geo == dict(emb=384, head=6, layer=12, mlp_ratio=4)
    target = shrink.macs_target(0.36, **geo)
    xp, yp = shrink.search_policy(m, [(img, lab)], nr, hr, 0.36, 3, 0, 0.5, dev, seed=3)
    assert xp.shape == (3, 24) and yp.shape == (3,) and all(0.0 <= y <= 100.0 for y in yp)
    for row in xp:
        assert abs(flops.macs_g(neuron_sparsity=row[:12], head_sparsity=row[12:], **geo) - target) <= 0.02 * target
    xp2, _ = shrink.search_policy(m, [(img, lab)], nr, hr, 0.36, 3, 0, 0.5, dev, seed=3, physical=False)
    assert np.array_equal(xp, xp2)
    for blk in shrink._blocks(m):
        assert bool((blk.attn.gate == 1).all()) and bool((blk.mlp.gate == 1).all()) and getattr(blk, "_compact", None) is None
    with torch.no_grad():
        after = m(img)
    if isinstance(before, tuple):
        assert all(torch.equal(a, b) for a, b in zip(before, after))
    else:
        assert torch.equal(before, after)


def test_shrink_to_distill_sub_chain(tmp_path):
    """shrink.py writes the directory that distill_sub.py --shrink_checkpoint reads; no file is moved in between."""
    _need_gpu()
    import distill_sub
    import shrink as cli
    from devit_amd import shrink
    a = argparse.ArgumentParser(parents=[cli.get_args_parser()]).parse_args(
        ["--synthetic", "2", "--batch-size", "8", "--population", "3", "--shrink_ratio", "0.36", "--neuron_shrinking", "--head_shrinking",
         "--output_dir", str(tmp_path / "s")])
    xp, yp = cli.main(a)
    assert xp.shape == (3, 24) and yp.shape == (3,)
    ns, hs = shrink.read_shrink_checkpoint(a.shrink_dir)
    assert len(ns) == 12 and len(hs) == 12
    d = argparse.ArgumentParser(parents=[distill_sub.get_args_parser()]).parse_args(
        ["--synthetic", "2", "--shrink_checkpoint", a.shrink_dir, "--neuron_shrinking", "--head_shrinking", "--epochs", "1",
         "--batch-size", "4", "--teacher-model", "deit_base_distilled_patch16_224", "--warmup-epochs", "0", "--output_dir", str(tmp_path / "d")])
    distill_sub.main(d)
    line = json.loads(open(os.path.join(d.output_dir, "sub-dataset0", "log.txt")).read().splitlines()[-1])
    assert line["train_loss"] == line["train_loss"] and "test_acc1" in line
