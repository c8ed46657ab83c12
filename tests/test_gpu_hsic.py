"""The ranking kernels of the shrink stage (csrc/hsic.hip) against a float64 CPU evaluation of the repository's own
restatement (shrink._hsic / _gauss_mix on .double() tensors), the golden ranks, a real forward's activations, the policy
search and the shrink.py -> distill_sub.py chain.

Bar for rel, red and the final scores: |score - ref| <= 2e-5 * max|ref| on identical inputs rounded to the type fed to the
kernel (the project's fp32-kernel bar; the fp32 torch statement sits at 1e-7 .. 2.6e-7 of it on the
CPU); act is a plain sum and is held to 1e-6 relative.  Every measured deviation goes through conftest.chk under a name that starts
with "hsic", so it lands in the session's parity margins; profiles/hsic_parity.json is the committed copy of those rows.

Those bars are normed by the largest score of a call and see the composed result only.  The second half of this file (from "per-element bounds"
on) holds every stage on its own -- the packed workspace, every element of Kmix - 1 and of W, rel, act and red -- below the bounds tests/_hsic_model.py
counts from the kernel source, at the seams of the kernels' tiles, through the C ABI with poisoned memory and guarded outputs; its rows are named
"hsic/<kernel>/<case>/<output>" and profiles/hsic_bounds_margins.json is their committed copy."""
import argparse
import json
import math
import os

import numpy as np
import pytest
import torch

import _hsic_model as HM
from _hsic_model import F32, ratio
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


# ============================================================================================ per-element bounds (tests/_hsic_model.py)
# Every stage of csrc/hsic.hip against the float64 statement applied to the fp32 values the stage in front of it left on the device, element by
# element, under bounds counted from the kernel source; launched through the C ABI with a workspace of exactly the queried size, NaN in the workspace,
# in every output and in whatever of X the operand description does not name, and sentinel elements in front of and behind every written buffer.
SENT, GUARD = -123.0, 64          # 64 fp32 guard elements are 256 bytes: the live part of a guarded buffer keeps the allocation's alignment


@pytest.fixture(scope="module")
def dev():
    d = _need_gpu()
    from devit_amd import _lib
    _lib.require_device(torch.zeros(1, device=d))
    return d


def _abi(name, *args):
    from devit_amd import _lib
    return _lib.call(name, *[_lib.ptr(a) if isinstance(a, torch.Tensor) else a for a in args], _lib.stream_ptr())


class Guarded:
    """n fp32 elements, NaN, between two runs of GUARD sentinels that must come back bit for bit"""

    def __init__(self, dev, *shape):
        self.n = int(np.prod(shape))
        self.flat = torch.full((GUARD + self.n + GUARD,), SENT, dtype=F32, device=dev)
        self.v = self.flat[GUARD:GUARD + self.n].view(*shape)
        self.v.fill_(math.nan)

    def intact(self):
        want = torch.full((GUARD,), SENT, dtype=F32, device=self.flat.device).view(torch.int32)
        ok = torch.equal(self.flat[:GUARD].view(torch.int32), want) and torch.equal(self.flat[GUARD + self.n:].view(torch.int32), want)
        assert ok, "a write outside an output's extent (guard elements changed)"
        return True

    def untouched(self):
        return self.intact() and bool(torch.isnan(self.v).all())


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _hold(tag, got, ref, bnd):
    r = ratio(got, ref, bnd)
    print(f"hsic/{tag} {r:.3f}")
    assert chk(r, 1.0, name=f"hsic/{tag}"), f"hsic/{tag}: worst |err| / bound {r:.3f}"


def _place(X, c, dev, layout=None):
    """X in a NaN-filled buffer at the case's strides and base offset -> (the view, batch stride, token stride)"""
    off, sb, sn, total = HM.strides_of(dict(c, layout=layout or c["layout"]))
    buf = torch.full((total,), math.nan, dtype=X.dtype, device=dev)
    view = buf.as_strided(tuple(X.shape), (sb, sn, 1), off)
    view.copy_(X.to(dev))
    return view, sb, sn


def _elem(dtype):
    from devit_amd import _lib
    return {torch.bfloat16: _lib.HSIC_BF16, torch.float16: _lib.HSIC_F16, torch.float32: _lib.HSIC_F32}[dtype]


def _scores(dev, c, X, W, layout=None, want_act=True, want_kmix=True):
    """one launch of devit_hsic_scores -> dict of Guarded rel, act, kmix1, ws (all intact), with ws exactly the queried bytes"""
    B, N, units, group = c["B"], c["N"], c["units"], c["group"]
    view, sb, sn = _place(X, c, dev, layout)
    need = HM.workspace_bytes(B, N, units)
    o = dict(rel=Guarded(dev, units), act=Guarded(dev, units) if (want_act and group == 1) else None,
             kmix1=Guarded(dev, units, B, B) if want_kmix else None, ws=Guarded(dev, units, N, HM.padded(B)))
    _abi("devit_hsic_scores", view, _elem(X.dtype), B, N, units, group, sb, sn, W, o["rel"].v, o["act"].v if o["act"] else None,
         o["kmix1"].v if o["kmix1"] else None, o["ws"].v, need)
    torch.cuda.synchronize()
    assert all(b.intact() for b in o.values() if b is not None)
    return o


_SCORE_RUNS = {}


def _score_run(dev, name):
    """the full launch of a score case, made once (test_head_pairs_bounds feeds on the kmix1 of the group cases)"""
    if name not in _SCORE_RUNS:
        c = HM.case_by_name(name)
        i = HM.score_inputs(c)
        _SCORE_RUNS[name] = (c, i, i["W"].to(dev), _scores(dev, c, i["X"], i["W"].to(dev)))
    return _SCORE_RUNS[name]


@pytest.mark.parametrize("name", [c["name"] for c in HM.score_cases()])
def test_scores_hold_per_element_bounds(dev, name):
    c, i, W, o = _score_run(dev, name)
    B, group, units = c["B"], c["group"], c["units"]
    X = i["X"]
    ws, k = o["ws"].v, o["kmix1"].v
    # pack: the workspace is features(X), unit-major, zero in samples B .. Bp
    ref, bnd = HM.pack_bounds(X.to(dev), group)
    if group == 1:
        assert torch.equal(ws[:, :, :B], X.to(dev).float().permute(2, 1, 0)), "pack (group == 1) is a conversion and a copy"
    else:
        _hold(f"pack/{name}/ws", ws[:, :, :B], ref, bnd)
    assert bool((ws[:, :, B:] == 0).all()), "samples B .. Bp of the workspace are zero"
    # pair: kmix1 per element from the workspace as it stands; rel and act from the device's own kmix1 / workspace
    kref, kbnd = HM.kmix1_bounds(ws[:, :, :B])
    _hold(f"pair/{name}/kmix1", k, kref, kbnd)
    assert torch.equal(k, k.transpose(1, 2)) and bool((torch.diagonal(k, dim1=1, dim2=2) == 0).all())
    _hold(f"pair/{name}/rel", o["rel"].v, *HM.rel_bounds(k, W))
    if group == 1:
        _hold(f"pair/{name}/act", o["act"].v, *HM.act_bounds(ws))
    for u in range(4, units, 6):                                    # a masked unit: exactly zero everywhere
        assert not bool(k[u].any()) and float(o["rel"].v[u]) == 0.0 and (group != 1 or float(o["act"].v[u]) == 0.0)
    # what does not depend on numerics: optional outputs left out, a second launch, the contiguous form
    o2 = _scores(dev, c, X, W, want_kmix=False)
    assert _same_bits(o2["rel"].v, o["rel"].v) and (group != 1 or _same_bits(o2["act"].v, o["act"].v)), "kmix1 == NULL changes rel or act"
    o3 = _scores(dev, c, X, W, want_act=False)
    assert _same_bits(o3["rel"].v, o["rel"].v) and _same_bits(o3["kmix1"].v, k), "act == NULL changes rel or kmix1"
    o4 = _scores(dev, c, X, W, layout="contig")                     # for a contiguous case: the second identical launch
    for key in ("rel", "act", "kmix1", "ws"):
        assert o[key] is None or _same_bits(o4[key].v, o[key].v), f"{key}: the contiguous form / a second launch gives other bits"


def _head_pairs(dev, k):
    H, B = k.shape[0], k.shape[1]
    red = Guarded(dev, H)
    _abi("devit_hsic_head_pairs", k, H, B, red.v)
    torch.cuda.synchronize()
    assert red.intact()
    return red


@pytest.mark.parametrize("name", [c["name"] for c in HM.head_cases()] + ["synthetic"])
def test_head_pairs_bounds(dev, name):
    if name == "synthetic":
        k = HM.synthetic_kmix1().to(dev)
    else:
        k = _score_run(dev, name)[3]["kmix1"].v
    before = k.clone()
    red = _head_pairs(dev, k)
    _hold(f"head_pairs/{name}/red", red.v, *HM.red_bounds(k))
    assert _same_bits(_head_pairs(dev, k).v, red.v) and torch.equal(k, before)


def _target(dev, c, y):
    B, C = c["B"], c["C"]
    ybuf = torch.full((GUARD + B * C + GUARD,), math.nan, dtype=F32, device=dev)          # NaN around the operand
    yv = ybuf[GUARD:GUARD + B * C].view(B, C)
    yv.copy_(y.to(dev))
    W, ws = Guarded(dev, B, B), Guarded(dev, B, C)
    _abi("devit_hsic_target", yv, B, C, c["softmax"], W.v, ws.v, B * C * 4)
    torch.cuda.synchronize()
    assert W.intact() and ws.intact()
    return W


@pytest.mark.parametrize("name", [c["name"] for c in HM.target_cases()])
def test_target_holds_per_element_bounds(dev, name):
    c = HM.case_by_name(name)
    y = HM.target_inputs(c)
    W = _target(dev, c, y)
    _hold(f"target/{name}/W", W.v, *HM.target_bounds(y.to(dev), c["softmax"]))
    assert torch.equal(W.v, W.v.t()), "both triangles of W are the same products in the same order"
    assert _same_bits(_target(dev, c, y).v, W.v)
    if c["C"] == 1 and c["softmax"]:
        assert not bool(W.v.any())                                   # one class: p = 1, z = 0, W = 0 exactly


def test_refused_calls_write_nothing(dev):
    """the return codes are the CPU ABI test's; here: every output of a refused call still holds its NaN fill, the guards their sentinels"""
    from devit_amd._lib import DevitError
    c = HM.case_by_name("B65_N3_u6_g1_bf16_token_pad")
    i = HM.score_inputs(c)
    B, N, units = c["B"], c["N"], c["units"]
    view, sb, sn = _place(i["X"], c, dev)
    W = i["W"].to(dev)
    need = HM.workspace_bytes(B, N, units)
    el = _elem(i["X"].dtype)
    rel, act, k, ws = Guarded(dev, units), Guarded(dev, units), Guarded(dev, units, B, B), Guarded(dev, units, N, HM.padded(B))
    bad = [(view, el, B, N, units, 1, sb, sn, W, rel.v, act.v, k.v, ws.v, need - 4),                  # workspace four bytes short
           (view, el, B, N, units, 1, sb, sn, W, rel.v, act.v, k.v, ws.flat[GUARD + 1:], need),       # workspace not 16-byte aligned
           (view, el, B, N, units, 1, sb, units - 1, W, rel.v, act.v, k.v, ws.v, need),               # token rows overlap
           (view, el, B, N, units, 1, (N - 1) * sn + units - 1, sn, W, rel.v, act.v, k.v, ws.v, need),          # samples overlap
           (view, el, B, N, units // 2, 2, sb, sn, W, rel.v, act.v, k.v, ws.v, need),                 # act with group > 1
           (view, 3, B, N, units, 1, sb, sn, W, rel.v, act.v, k.v, ws.v, need),                       # element type
           (view, el, 257, N, units, 1, sb, sn, W, rel.v, act.v, k.v, ws.v, need),                    # batch
           (view, el, B, 0, units, 1, sb, sn, W, rel.v, act.v, k.v, ws.v, need)]                      # no token
    for args in bad:
        with pytest.raises(DevitError):
            _abi("devit_hsic_scores", *args)
    tc = HM.case_by_name("B65_C257_softmax")
    y = HM.target_inputs(tc).to(dev)
    Wo, tws, red = Guarded(dev, 65, 65), Guarded(dev, 65, 257), Guarded(dev, 17)
    for args in [(y, 65, 257, 1, Wo.v, tws.v, 65 * 257 * 4 - 4), (y, 1, 257, 1, Wo.v, tws.v, 65 * 257 * 4), (y, 65, 0, 1, Wo.v, tws.v, 65 * 257 * 4)]:
        with pytest.raises(DevitError):
            _abi("devit_hsic_target", *args)
    kk = HM.synthetic_kmix1().to(dev)
    for args in [(kk, 17, 65, red.v), (kk, 1, 65, red.v), (kk, 3, 257, red.v), (kk, 3, 1, red.v)]:
        with pytest.raises(DevitError):
            _abi("devit_hsic_head_pairs", *args)
    torch.cuda.synchronize()
    assert all(b.untouched() for b in (rel, act, k, ws, Wo, tws, red))
