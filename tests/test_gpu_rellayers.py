"""Relation losses on chosen layer pairs on a real MI355X: engine.distill_forward(relation_layers=...), TeacherLookahead(relation_layers=...),
distill_sub.py --relation-layers.

`dedeit` under `deit_base_distilled_patch16_224`, C = 25, fixed DropPath scales, against the CPU helper tests/_rellayers_model.py (pinned to
tests/_imgsize_model.distill_step at the middle pair by tests/test_rellayers_host.py).  S = 64 (N = 18 rows an image: fewer than one tile) with
the odd batch B = 3 for the selections (0, 5, 11), `last` and `all`; S = 224 (N = 198) with B = 2 for `all`, where twelve packed q/k/v buffers
carry the zeroed overhang rows the relation kernels read.  Bars are the project's own (test_gpu_imgsize.py::test_step_at_112_vs_helper):
precision="f32" losses 1e-4, gradient norms and slices 1e-3; bf16 losses 5e-4, gradient norms 3e-3, slices 1.5e-2 -- measured there for the
middle pair alone; a bf16 figure of another layer that needs its own bar has it in BF16_LAYER_BARS / BF16_SUM_BARS with the measurement beside it (committed
rows: profiles/rellayers_parity_margins.json)."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import _imgsize_model as IM
import _rellayers_model as RM
from oracle import devit_oracle as O
from oracle.detgen import det_array, det_labels
from conftest import chk

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C = 25
GS, GT = O.GEOMETRY["dedeit"], O.GEOMETRY["deit_base_distilled_patch16_224"]
LOSSES = ("loss", "cls_loss", "q_loss", "k_loss", "v_loss")
GAMA = (0.2, 0.1, 0.3)
# bf16 loss figures over the project's 5e-4 get a bar of their own, about twice what was measured against the helper on the MI355X (the 5e-4 was
# measured for the middle pair at S = 112 / 224; at S = 64, B = 3 a layer's loss is a mean over 3 x 6 x 18 x 18 Gram entries only, and block 5's k
# loss itself measures 1.17e-3).  Per layer, "S<size>_L<student block>_<q|k|v>": the measurement is the same in every selection that holds the
# layer.  Measured: S64 L0 q 5.1e-4; L1 q 5.6e-4; L2 q 9.1e-4, k 1.30e-3; L3 k 1.14e-3; L4 q 5.8e-4, v 8.5e-4; L5 k 1.17e-3; L6 q 1.34e-3, k 6.0e-4,
# v 9.9e-4; L7 k 1.22e-3; L8 k 1.83e-3, v 9.5e-4; L9 q 1.01e-3, v 1.01e-3; L10 q 6.7e-4, v 1.05e-3; L11 k 8.7e-4, v 8.9e-4; S224 L6 v 5.6e-4, L7 k 5.6e-4,
# L11 v 5.9e-4.  Every other layer figure, and every figure at precision="f32", meets the project's bar.
BF16_LAYER_BARS = {"S64_L0_q": 1.1e-3, "S64_L1_q": 1.2e-3, "S64_L2_q": 1.9e-3, "S64_L2_k": 2.6e-3, "S64_L3_k": 2.3e-3, "S64_L4_q": 1.2e-3,
                   "S64_L4_v": 1.8e-3, "S64_L5_k": 2.4e-3, "S64_L6_q": 2.7e-3, "S64_L6_k": 1.3e-3, "S64_L6_v": 2.0e-3, "S64_L7_k": 2.5e-3,
                   "S64_L8_k": 3.7e-3, "S64_L8_v": 2.0e-3, "S64_L9_q": 2.1e-3, "S64_L9_v": 2.1e-3, "S64_L10_q": 1.4e-3, "S64_L10_v": 2.2e-3,
                   "S64_L11_k": 1.8e-3, "S64_L11_v": 1.8e-3, "S224_L6_v": 1.2e-3, "S224_L7_k": 1.2e-3, "S224_L11_v": 1.2e-3}
# ... and the sums over a selection's layers / 12 (q_loss, k_loss, v_loss) that are over it.  Measured: (0, 5, 11) k 9.1e-4, v 6.0e-4; last k 8.7e-4,
# v 8.9e-4 (block 11's own figures); all v 5.7e-4
BF16_SUM_BARS = {"rellayers_S64_0_5_11_bf16_k_loss": 1.9e-3, "rellayers_S64_0_5_11_bf16_v_loss": 1.3e-3, "rellayers_S64_last_bf16_k_loss": 1.8e-3,
                 "rellayers_S64_last_bf16_v_loss": 1.8e-3, "rellayers_S64_all_bf16_v_loss": 1.2e-3}


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


_state_cache = {}


def fresh_model(name, S, dev, **kw):
    import devit_amd
    geom = O.GEOMETRY[name]
    if (name, S) not in _state_cache:
        _state_cache[(name, S)] = IM.make_state(geom, C, "T" if geom["embed_dim"] == 768 else "S", S)
    st = _state_cache[(name, S)]
    m = devit_amd.create_model(name, num_classes=C, img_size=S, **kw)
    m.load_state_dict(st)
    return m.to(dev), st


_model_cache = {}


def model_at(name, S, dev, **kw):
    """(HIP model on the device, its CPU state): built once per (name, size)."""
    key = (name, S, tuple(sorted(kw.items())))
    if key not in _model_cache:
        _model_cache[key] = fresh_model(name, S, dev, **kw)
    return _model_cache[key]


def frozen(t):
    t.eval()
    for p in t.parameters():
        p.requires_grad_(False)
    return t


_setup_cache = {}


def setup(dev, S, B):
    """models, one deterministic batch with mixed soft targets, fixed DropPath scales (some branch dropped for some sample): once per shape"""
    if (S, B) not in _setup_cache:
        s, st_s = model_at("dedeit", S, dev, drop_path_rate=0.1)
        t, st_t = model_at("deit_base_distilled_patch16_224", S, dev)
        frozen(t)
        img = torch.from_numpy(det_array(f"rellayers/step{S}", (B, 3, S, S)))
        y1, y2 = det_labels("rellayers/sy1", B, C), det_labels("rellayers/sy2", B, C)
        oh = lambda y: torch.full((B, C), 0.1 / C).scatter_(1, torch.from_numpy(y)[:, None], 1 - 0.1 + 0.1 / C)
        soft = oh(y1) * 0.7 + oh(y2) * 0.3
        dps = IM.dp_scales_for(f"rellayers/step{S}", B)
        assert any(float(a.min()) == 0.0 or float(b.min()) == 0.0 for a, b in dps)
        d = [(a.to(dev).contiguous(), b.to(dev).contiguous()) for a, b in dps]
        _setup_cache[(S, B)] = dict(s=s, t=t, st_s=st_s, st_t=st_t, img=img, soft=soft, dps=dps, x=img.to(dev), y=soft.to(dev), d=d)
    return _setup_cache[(S, B)]


_ref_cache = {}


def gated_state(st, head_gates, neuron_gates):
    """The gated student as the ungated one on masked weights: a 0/1 head gate on the head outputs is a 0/1 mask on proj's columns, a neuron gate
    behind GELU one on fc2's columns (models/de_vit.py:77-79, 43-45) -- the q/k/v of a masked head still enter the relation loss."""
    out = dict(st)
    for i, (hg, ng) in enumerate(zip(head_gates, neuron_gates)):
        out[f"blocks.{i}.attn.proj.weight"] = st[f"blocks.{i}.attn.proj.weight"] * hg.repeat_interleave(64)[None, :]
        out[f"blocks.{i}.mlp.fc2.weight"] = st[f"blocks.{i}.mlp.fc2.weight"] * ng[None, :]
    return out


def reference(dev, S, B, layers, gates=None):
    """the helper's step and gradients for one selection: computed once, never written"""
    key = (S, B, layers if isinstance(layers, str) else tuple(layers), gates is not None)
    if key not in _ref_cache:
        z = setup(dev, S, B)
        leaves = {k: v.clone().requires_grad_(True) for k, v in z["st_s"].items()}
        st = leaves if gates is None else gated_state(leaves, *gates)
        ref = RM.distill_step(st, GS, z["st_t"], GT, z["img"], z["soft"], layers=layers, gama=GAMA, dp_scales=z["dps"])
        ref["loss"].backward()
        _ref_cache[key] = (ref, {k: v.grad for k, v in leaves.items()})
    return _ref_cache[key]


def one_k_slice(monkeypatch):
    """Bit-for-bit comparisons of two backward passes need sums with ONE order: the patch-embedding weight gradient is a split-K GEMM whose slices
    add their partial sums with fp32 atomics in arrival order (tests/test_gpu_hid.py::one_k_slice).  With one slice every element is one add."""
    from devit_amd import ops
    monkeypatch.setattr(ops, "split_k_for", lambda out_rows, out_cols, ksteps: 1)


def run_step(s, t, z, **kw):
    from devit_amd import engine
    s.train()
    for p in s.parameters():
        p.grad = None
    out = engine.distill_forward(s, t, z["x"], z["y"], gama=GAMA, kind="hard", alpha=0.5, tau=1.0, dp_scales=z["d"], **kw)
    out["loss"].backward()
    torch.cuda.synchronize()
    grads = {n: p.grad.detach().clone() for n, p in s.named_parameters()}
    for p in s.parameters():
        p.grad = None
    return out, grads


def same_bits(a, b, ga, gb, keys=LOSSES):
    bad = [k for k in keys if not torch.equal(a[k], b[k])]
    bad += [n for n in ga if not torch.equal(ga[n], gb[n])]
    return bad


SLICES = [("head.weight", lambda g: g), ("blocks.5.attn.qkv.weight", lambda g: g[::48]), ("blocks.0.mlp.fc1.weight", lambda g: g[::64]),
          ("blocks.11.mlp.fc2.weight", lambda g: g[::16]), ("pos_embed", lambda g: g[0]), ("cls_token", lambda g: g),
          ("patch_embed.proj.weight", lambda g: g[::16].reshape(-1, 768)), ("norm.weight", lambda g: g),
          # blocks that get relation gradient from the new selections only
          ("blocks.0.attn.qkv.weight", lambda g: g[::48]), ("blocks.11.attn.qkv.weight", lambda g: g[::48])]


def check_step(out, grads_hip, ref, grads, precision, tag):
    """the five losses, rel_layers per entry, all gradient norms, the gradient slices: every figure through chk, the failures collected"""
    loss_bar, norm_bar, slice_bar = (1e-4, 1e-3, 1e-3) if precision == "f32" else (5e-4, 3e-3, 1.5e-2)
    fails = []

    def loss_chk(got, want, name, own=None):
        e = abs(float(got) - float(want)) / abs(float(want))
        print(f"{name}: {float(got):.6f} vs {float(want):.6f} rel {e:.3e}")
        if not chk(e, own if (own is not None and precision == "bf16") else loss_bar, name=name):
            fails.append((name, e))
    size = re.match(r"rellayers_(S\d+)_", tag).group(1)
    for k in LOSSES:
        loss_chk(out[k].detach(), ref[k].detach(), f"{tag}_{precision}_{k}", BF16_SUM_BARS.get(f"{tag}_{precision}_{k}"))
    pairs = ref["pairs"]
    assert tuple(out["rel_layers"].shape) == (len(pairs), 3)
    got = out["rel_layers"].detach().float().cpu()
    for i, (sb, _) in enumerate(pairs):
        for j, c in enumerate("qkv"):
            assert float(ref["rel_layers"][i, j]) > 0.05            # (a relative error means something: no layer is near zero, none is left out)
            loss_chk(got[i, j], ref["rel_layers"][i, j], f"{tag}_{precision}_rel_L{sb}_{c}", BF16_LAYER_BARS.get(f"{size}_L{sb}_{c}"))
    names = list(grads_hip)
    assert len(names) == 155
    gn = np.array([grads_hip[n].norm().item() for n in names])
    rn = np.array([grads[n].norm().item() for n in names])
    if precision == "f32":
        worst = float(np.abs(gn - rn).max() / rn.max())
        if not chk(worst, norm_bar, name=f"{tag}_f32_grad_norms"):
            fails.append(("grad norms", worst))
    else:
        chk(float((np.abs(gn - rn) / (rn + 1e-3 * rn.max())).max()), norm_bar, name=f"{tag}_bf16_grad_norms")
        bad = np.abs(gn - rn) > norm_bar * rn + 3e-6 * rn.max()
        if bad.any():
            fails.append([(names[i], gn[i], rn[i]) for i in np.nonzero(bad)[0][:8]])
    for n, cut in SLICES:
        e = rel(cut(grads_hip[n]), cut(grads[n]))
        print(f"{tag} {precision} grad {n}: rel {e:.3e}")
        if not chk(e, slice_bar, name=f"{tag}_{precision}_g_{n}"):
            fails.append((n, e))
    return fails


def tag_of(layers):
    return layers if isinstance(layers, str) else "_".join(str(v) for v in layers)


# ------------------------------------------------------------------------------------------ a, b: the step against the helper
@pytest.mark.parametrize("precision", ["f32", "bf16"])
@pytest.mark.parametrize("layers", [(0, 5, 11), "last", "all"], ids=tag_of)
def test_step_at_64_vs_helper(dev, layers, precision):
    z = setup(dev, 64, 3)
    ref, grads = reference(dev, 64, 3, layers)
    s, t = z["s"], z["t"]
    try:
        s.precision = t.precision = precision
        out, g = run_step(s, t, z, relation_layers=layers)
        fails = check_step(out, g, ref, grads, precision, f"rellayers_S64_{tag_of(layers)}")
        assert not fails, fails
    finally:
        s.precision = t.precision = "bf16"


def test_step_at_224_all_layers(dev):
    """N = 198: every one of the twelve packed q/k/v buffers of each model carries the zeroed overhang rows (qkv_pad_rows)"""
    z = setup(dev, 224, 2)
    ref, grads = reference(dev, 224, 2, "all")
    assert float(ref["rel_layers"].min()) > 1.0
    out, g = run_step(z["s"], z["t"], z, relation_layers="all")
    assert z["s"].qkv_pad_layers == set(range(12)) and z["t"].qkv_pad_layers == set(range(12))
    fails = check_step(out, g, ref, grads, "bf16", "rellayers_S224_all")
    assert not fails, fails


# ------------------------------------------------------------------------------------------ c: the default
def test_none_mid_and_block_5_are_one_step(dev, monkeypatch):
    one_k_slice(monkeypatch)
    z = setup(dev, 64, 3)
    o0, g0 = run_step(z["s"], z["t"], z)
    assert set(o0) == {"loss", "cls_loss", "q_loss", "k_loss", "v_loss", "logits", "teacher_logits"}      # the step as it was, dict and all
    for sel in ("mid", (5,), ["mid"]):
        o, g = run_step(z["s"], z["t"], z, relation_layers=sel)
        assert same_bits(o0, o, g0, g) == [], sel
        assert tuple(o["rel_layers"].shape) == (1, 3)
        assert torch.equal(o["rel_layers"][0] / 12, torch.stack([o[k] for k in ("q_loss", "k_loss", "v_loss")]).detach())
        assert torch.equal(o["logits"][0], o0["logits"][0]) and torch.equal(o["teacher_logits"], o0["teacher_logits"])


# ------------------------------------------------------------------------------------------ d: with the other families on
def test_other_families_follow_the_selection(dev):
    """hid_gama, qkv_ce_gama, qkv_cross_gama > 0 at (2, 5): each extra loss is the list function on the models' own outputs of those layers"""
    from devit_amd import engine, losses
    s, _ = model_at("dedeit", 64, dev, drop_path_rate=0.0)           # (no DropPath: the model's own forward is the step's)
    t = setup(dev, 64, 3)["t"]
    z = setup(dev, 64, 3)
    s.train()
    for m in (s, t):
        m.qkv_pad_layers, m.enc_layers = None, None                  # a plain forward: every block's q/k/v padded, every 'encoder' output
    with torch.no_grad():
        so = s(z["x"], output_qkv=True, output_encoders=True)
        to = t(z["x"], output_qkv=True, output_encoders=True)
        want = {"hid_loss": losses.cal_hid_relation_loss([so["encoder"][i] for i in (2, 5)], [to["encoder"][i] for i in (2, 5)]),
                "qkv_ce_loss": losses.cal_qkv_loss([so["qkv"][i] for i in (2, 5)], [to["qkv"][i] for i in (2, 5)], layout="view"),
                "qkv_cross_loss": losses.cal_qkv_loss2([so["qkv"][i] for i in (2, 5)], [to["qkv"][i] for i in (2, 5)], layout="view")}
        one = {k: float(f([so[w][5]], [to[w][5]])) for k, f, w in (("hid_loss", losses.cal_hid_relation_loss, "encoder"),
                                                                   ("qkv_ce_loss", losses.cal_qkv_loss, "qkv"))}
    for p in s.parameters():
        p.grad = None
    w = dict(hid_gama=0.5, qkv_ce_gama=0.25, qkv_cross_gama=0.125)
    out = engine.distill_forward(s, t, z["x"], z["y"], gama=GAMA, relation_layers=(2, 5), **w)
    assert s.qkv_pad_layers == {2, 5} and t.qkv_pad_layers == {2, 5}
    for k, v in want.items():
        e = abs(float(out[k].detach()) - float(v)) / abs(float(v))
        print(f"rellayers families {k}: {float(out[k].detach()):.6f} vs {float(v):.6f} rel {e:.3e}")
        assert chk(e, 1e-6, name=f"rellayers_families_{k}"), (k, e)
    for k, v in one.items():                                         # ... and not the middle pair's alone
        assert abs(float(out[k].detach()) - v) > 1e-4 * abs(v), k
    total = (out["cls_loss"].double() + (out["rel_layers"].double() * torch.tensor(GAMA, device=dev).double() / 12).sum()
             + 0.5 * out["hid_loss"].double() + 0.25 * out["qkv_ce_loss"].double() + 0.125 * out["qkv_cross_loss"].double())
    assert chk(abs(float(out["loss"].detach()) - float(total.detach())) / abs(float(total.detach())), 1e-6, name="rellayers_families_total")
    out["loss"].backward()
    torch.cuda.synchronize()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in s.parameters())
    for p in s.parameters():
        p.grad = None


# ------------------------------------------------------------------------------------------ e: the lean tail follows the selection
def test_lean_tail_follows_the_selection(dev, monkeypatch):
    """the launches the library reports (tests/test_gpu_tail_launches.py): without block 11 both models run their last block through the tail
    entry points (attention of the token rows' queries), with it in full; the logits are the same bits"""
    from devit_amd import de_vit, ops
    assert de_vit.LEAN_TAIL
    z = setup(dev, 64, 3)
    s, t = z["s"], z["t"]
    recs = []

    def record(phase, stream, i):
        if phase == 0:
            recs.append((i.name.decode(), i.width))
    monkeypatch.setattr(ops, "_record", record)            # (the backward runs on autograd's thread: ops.call() observes on whichever thread calls)
    monkeypatch.setattr(ops, "PROFILE", [])

    def launches(sel):
        del recs[:]
        out, _ = run_step(s, t, z, relation_layers=sel)
        n = lambda name, width: sum(1 for r in recs if r == (name, width))
        return out, {(k, wd): n("devit_attn_" + k, wd) for k in ("fwd", "fwd_rows", "bwd", "bwd_rows") for wd in (384, 768)}
    lean, a = launches((0, 5))
    full, b = launches((5, 11))
    assert a == {("fwd", 384): 11, ("fwd_rows", 384): 1, ("bwd", 384): 11, ("bwd_rows", 384): 1,
                 ("fwd", 768): 11, ("fwd_rows", 768): 1, ("bwd", 768): 0, ("bwd_rows", 768): 0}, a
    assert b == {("fwd", 384): 12, ("fwd_rows", 384): 0, ("bwd", 384): 12, ("bwd_rows", 384): 0,
                 ("fwd", 768): 12, ("fwd_rows", 768): 0, ("bwd", 768): 0, ("bwd_rows", 768): 0}, b
    assert torch.equal(lean["logits"][0], full["logits"][0]) and torch.equal(lean["logits"][1], full["logits"][1])
    assert torch.equal(lean["teacher_logits"], full["teacher_logits"])
    assert torch.equal(lean["rel_layers"][1], full["rel_layers"][0])                 # block 5's row, in both


# ------------------------------------------------------------------------------------------ f: look-ahead
def test_lookahead_for_a_selection(dev, monkeypatch):
    from devit_amd import engine
    one_k_slice(monkeypatch)
    z = setup(dev, 64, 3)
    s, t, x = z["s"], z["t"], z["x"]
    sel = (0, 5, 11)
    inside, gi = run_step(s, t, z, relation_layers=sel)
    look = engine.TeacherLookahead(t, relation_layers=sel, student_depth=12)
    look.submit(x, defer=True)
    run_step(s, t, z, relation_layers="mid")               # a step in between leaves its own request on the teacher: the launch makes its own again
    t_out = look.take(x)
    assert t_out["relation_layers"] == sel and t_out["qkv"][11] is not None and t.qkv_pad_layers == set(sel)
    ahead, ga = run_step(s, t, z, relation_layers=sel, teacher_outputs=t_out)
    assert same_bits(inside, ahead, gi, ga) == [] and torch.equal(inside["rel_layers"], ahead["rel_layers"])
    # outputs made for another selection, and an entry that is not there
    mid = engine.TeacherLookahead(t)
    mid.submit(x)
    t_mid = mid.take(x)
    with pytest.raises(RuntimeError, match=r"(?s)\[11\].*\[5\]"):
        engine.distill_forward(s, t, x, z["y"], dp_scales=z["d"], relation_layers="last", teacher_outputs=t_mid)
    bare = {k: v for k, v in t_mid.items() if k != "relation_layers"}                  # (someone's own dict: the lean teacher's block 11 is None)
    assert bare["qkv"][11] is None
    with pytest.raises(RuntimeError, match=r"(?s)\[11\].*teacher's.*\[11\]"):
        engine.distill_forward(s, t, x, z["y"], dp_scales=z["d"], relation_layers="last", teacher_outputs=bare)
    plain = engine.TeacherLookahead(t, relation_layers=sel, student_depth=12)          # hid=False under hid_gama > 0
    plain.submit(x)
    with pytest.raises(RuntimeError, match="hid=True"):
        engine.distill_forward(s, t, x, z["y"], dp_scales=z["d"], relation_layers=sel, hid_gama=0.5, teacher_outputs=plain.take(x))
    for p in s.parameters():
        p.grad = None


# ------------------------------------------------------------------------------------------ g: nothing sticks to the model objects
def test_order_independence(dev, monkeypatch):
    """all, then mid, then (0, 5, 11) on the same objects: each as on fresh objects (a sticky qkv_pad_layers / hidden-state request shows here)"""
    one_k_slice(monkeypatch)
    z = setup(dev, 64, 3)
    used_s, _ = fresh_model("dedeit", 64, dev, drop_path_rate=0.1)
    used_t = frozen(fresh_model("deit_base_distilled_patch16_224", 64, dev)[0])
    for sel, kw in (("all", dict(hid_gama=0.5)), ("mid", {}), ((0, 5, 11), dict(hid_gama=0.5))):
        got, gg = run_step(used_s, used_t, z, relation_layers=sel, **kw)
        s, _ = fresh_model("dedeit", 64, dev, drop_path_rate=0.1)
        t = frozen(fresh_model("deit_base_distilled_patch16_224", 64, dev)[0])
        want, gw = run_step(s, t, z, relation_layers=sel, **kw)
        assert same_bits(want, got, gw, gg, keys=LOSSES + (("hid_loss",) if kw else ())) == [], sel
        assert torch.equal(want["rel_layers"], got["rel_layers"])
        pairs = {"all": set(range(12)), "mid": {5}}.get(sel, {0, 5, 11})
        assert used_s.qkv_pad_layers == pairs and used_t.qkv_pad_layers == pairs


# ------------------------------------------------------------------------------------------ h: other configurations
def test_compacted_student(dev):
    """shrink.compact(trainable=True, relation_layers=(0, 5)): blocks 0 and 5 keep every head in their GEMMs (the q/k/v of masked heads enter the
    relation loss), the others run 4 of 6; against the helper with the same gates.  Bars: test_gpu_model.py::test_training_through_compacted_blocks'
    (losses 2e-3, gradient norms 1e-2); a layer figure whose uncompacted bar at this size is wider (block 5's k) keeps that one."""
    from devit_amd import engine, shrink
    z = setup(dev, 64, 3)
    s, _ = fresh_model("dedeit", 64, dev, drop_path_rate=0.1)
    t = z["t"]
    gen = torch.Generator().manual_seed(17)
    hgs, ngs = [], []
    for blk in s.blocks:
        hm, nm = torch.ones(6), torch.ones(1536)
        hm[torch.randperm(6, generator=gen)[:2]] = 0
        nm[torch.randperm(1536, generator=gen)[:461]] = 0
        blk.attn.gate, blk.mlp.gate = hm.clone(), nm.clone()
        hgs.append(hm)
        ngs.append(nm)
    ref, grads = reference(dev, 64, 3, (0, 5), gates=(hgs, ngs))
    shrink.compact(s, trainable=True)
    with pytest.raises(RuntimeError, match=r"block 0.*relation_layers"):          # compacted for the middle pair: block 0 lost the masked heads' q/k/v
        engine.distill_forward(s, t, z["x"], z["y"], dp_scales=z["d"], relation_layers=(0, 5))
    shrink.uncompact(s)
    rep = shrink.compact(s, trainable=True, relation_layers=(0, 5))
    assert [r[1] for r in rep] == [6] + [4] * 4 + [6] + [4] * 6
    out, g = run_step(s, t, z, relation_layers=(0, 5))
    fails = []
    for k in LOSSES:
        e = abs(float(out[k].detach()) - float(ref[k].detach())) / abs(float(ref[k].detach()))
        print(f"rellayers compacted {k}: {float(out[k].detach()):.6f} vs {float(ref[k].detach()):.6f} rel {e:.3e}")
        if not chk(e, 2e-3, name=f"rellayers_compacted_{k}"):
            fails.append((k, e))
    for i, sb in enumerate((0, 5)):
        for j, c in enumerate("qkv"):
            e = abs(float(out["rel_layers"][i, j]) - float(ref["rel_layers"][i, j])) / float(ref["rel_layers"][i, j])
            if not chk(e, max(2e-3, BF16_LAYER_BARS.get(f"S64_L{sb}_{c}", 0.)), name=f"rellayers_compacted_rel_L{sb}_{c}"):
                fails.append((sb, c, e))
    names = list(g)
    gn = torch.stack([g[n].norm() for n in names]).cpu()
    rn = torch.stack([grads[n].norm() for n in names])
    chk(float(((gn - rn).abs() / (rn + 1e-3 * rn.max())).max()), 1e-2, name="rellayers_compacted_grad_norms")
    bad = (gn - rn).abs() > 1e-2 * rn + 1e-3 * rn.max()
    if bool(bad.any()):
        fails.append([(n, float(a), float(b)) for n, a, b, f in zip(names, gn, rn, bad) if f][:8])
    for i, hm in enumerate(hgs):                                                  # the relation loss reaches the masked heads of blocks 0 and 5 alone
        qw = g[f"blocks.{i}.attn.qkv.weight"].view(3, 6, 64, 384)[:, (hm == 0).to(dev)]
        assert (float(qw.abs().max()) == 0.0) == (i not in (0, 5)), i
    assert not fails, fails


def test_deterministic_step_twice(dev):
    from devit_amd import ops
    z = setup(dev, 64, 3)
    with ops.deterministic():
        a, ga = run_step(z["s"], z["t"], z, relation_layers=(0, 5, 11), hid_gama=0.5, qkv_ce_gama=0.25)
        b, gb = run_step(z["s"], z["t"], z, relation_layers=(0, 5, 11), hid_gama=0.5, qkv_ce_gama=0.25)
    assert same_bits(a, b, ga, gb, keys=LOSSES + ("hid_loss", "qkv_ce_loss")) == [] and torch.equal(a["rel_layers"], b["rel_layers"])


def _run_cli(script, argv, tmp_path, limit=240, ok=True):
    """One child-process run of a CLI under its own time limit -> its stdout."""
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.join(ROOT, script)] + argv + ["--output_dir", str(tmp_path)]
    r = subprocess.run(cmd, cwd=str(tmp_path), env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert (r.returncode == 0) == ok, (r.returncode, r.stdout[-3000:])
    return r.stdout


def test_distill_sub_cli_relation_layers(dev, tmp_path):
    out = _run_cli("distill_sub.py", ["--synthetic", "2", "--batch-size", "8", "--input-size", "64", "--epochs", "1", "--warmup-epochs", "0",
                                      "--model", "dedeit", "--teacher-model", "deit_base_distilled_patch16_224",
                                      "--relation-layers", "0", "5", "11"], tmp_path)
    m = re.search(r"\[Train\] Loss: ([-+0-9.einfa]+)", out)
    assert m and np.isfinite(float(m.group(1))), out[-2000:]
    ck = torch.load(next(tmp_path.rglob("checkpoint_temp.pth")), map_location="cpu", weights_only=False)
    assert ck["args"].relation_layers == (0, 5, 11)
    line = json.loads(next(tmp_path.rglob("log.txt")).read_text().splitlines()[-1])
    assert all(np.isfinite(line[f"train_{k}"]) and line[f"train_{k}"] > 0 for k in ("q_loss", "k_loss", "v_loss"))
