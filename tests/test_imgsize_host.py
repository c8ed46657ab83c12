"""Image sizes other than 224 (img_size / --input-size), host side, no GPU: construction, refusals, checkpoint loading with a resized
position grid, the CLI plumbing and the FLOP accounting; and the two pins of the size-general CPU helper the GPU tests compare against
(tests/_imgsize_model.py): the oracle at 224, bit for bit, and the reference's own VisionTransformer(img_size=48) through a golden."""
import argparse
import json
import os

import numpy as np
import pytest
import torch

import _imgsize_model as IM
from oracle import devit_oracle as O
from oracle.detgen import det_array

C = 25
GS = O.GEOMETRY["dedeit"]
SIZES = tuple(range(32, 225, 16))


def close(a, b, rtol=2e-5, atol=2e-6):           # the comparison of tests/test_oracle_golden.py
    a = a.detach().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    scale = max(float(np.abs(b).max()), 1e-30)
    err = float(np.abs(a - b).max())
    assert err <= atol + rtol * scale, f"max err {err:.3e} vs scale {scale:.3e}"


# ------------------------------------------------------------------------------------------ the helper's two pins
def test_helper_equals_oracle_at_224():
    st, so = IM.make_state(GS, C, "S", 224), O.make_state(GS, C, "S")
    assert list(st) == list(so) and all(torch.equal(st[k], so[k]) for k in so)
    img = torch.from_numpy(det_array("imgsize/img224", (2, 3, 224, 224)))
    with torch.no_grad():
        a, b = IM.forward(st, GS, img), O.forward(so, GS, img)
        at, bt = IM.forward(st, GS, img, training=True), O.forward(so, GS, img, training=True)
    assert torch.equal(a["output"], b["output"]) and torch.equal(at["output"][0], bt["output"][0]) and torch.equal(at["output"][1], bt["output"][1])
    assert all(torch.equal(x, y) for x, y in zip(a["qkv"][5], b["qkv"][5])) and torch.equal(a["encoder"][0], b["encoder"][0])
    assert torch.equal(a["last_tokens"][0], b["last_tokens"][0]) and torch.equal(a["last_tokens"][1], b["last_tokens"][1])


def test_helper_vs_reference_golden_at_48(golden):
    """The comparison test_oracle_golden.py applies to model_dedeit, on the reference's VisionTransformer(img_size=48) (11 tokens)."""
    g = golden("imgsize_dedeit48")
    st = IM.make_state(GS, C, "S", 48)
    assert len(st) == int(g["n_keys"]) == 155 and list(st["pos_embed"].shape) == g["pos_shape"].tolist() == [1, 11, 384]
    img = torch.from_numpy(det_array("imgsize/img48", (2, 3, 48, 48)))
    with torch.no_grad():
        o = IM.forward(st, GS, img, training=False)
        tr = IM.forward(st, GS, img, training=True)
    close(o["output"], g["logits"], rtol=5e-5)
    assert np.array_equal(o["output"].argmax(1).numpy(), g["top1"])
    close(tr["output"][0], g["train_cls"], rtol=5e-5); close(tr["output"][1], g["train_dist"], rtol=5e-5)
    q, k, v = o["qkv"][5]
    assert q.shape == (2, 6, 11, 64)
    close(q[:, :2], g["q5"], rtol=5e-5); close(k[:, :2], g["k5"], rtol=5e-5); close(v[:, :2], g["v5"], rtol=5e-5)
    close(o["encoder"][-1][:, :, ::8], g["enc_last"], rtol=5e-5)
    close(o["last_tokens"][0], g["last_cls"], rtol=5e-5); close(o["last_tokens"][1], g["last_dist"], rtol=5e-5)


# ------------------------------------------------------------------------------------------ construction
@pytest.mark.parametrize("name,ntok", [("dedeit", 2), ("devit", 1)])
def test_construction_at_every_size(name, ntok):
    import devit_amd
    with open(os.path.join(os.path.dirname(__file__), "golden", "statedict_keys.json")) as f:
        keys224 = [k for k, _ in json.load(f)["dedeit_keys"]]
    for S in SIZES:
        m = devit_amd.create_model(name, num_classes=C, img_size=S, depth=2)          # (depth 2: the front is what changes)
        G = S // 16
        assert m.patch_embed.img_size == (S, S) and m.patch_embed.grid_size == (G, G) and m.patch_embed.num_patches == G * G
        assert tuple(m.pos_embed.shape) == (1, G * G + ntok, 384) and m.num_tokens == ntok
        assert m.default_cfg["input_size"] == (3, S, S)
        assert tuple(m.patch_embed.proj.weight.shape) == (384, 3, 16, 16)
    # full depth: the keys, their order and every shape are the helper's, i.e. the reference's with another pos_embed
    for S in (32, 112, 224):
        sd = devit_amd.create_model("dedeit", num_classes=C, img_size=S).state_dict()
        assert [(k, tuple(v.shape)) for k, v in sd.items()] == IM.state_keys(GS, C, S)
        assert list(sd) == keys224 and len(sd) == 155


@pytest.mark.parametrize("kw", [dict(img_size=16), dict(img_size=100), dict(img_size=240), dict(img_size=(112, 224)), dict(patch_size=32),
                                dict(in_chans=1), dict(img_size=0)])
def test_unsupported_sizes_raise_at_construction(kw):
    import devit_amd
    with pytest.raises(NotImplementedError) as e:
        devit_amd.create_model("dedeit", num_classes=C, depth=1, **kw)
    assert "patch-embed kernels" in str(e.value)
    if kw.get("img_size") == 240:
        assert "227" in str(e.value) and "208" in str(e.value)          # the reason for the ceiling


def test_default_stays_224():
    import devit_amd
    m = devit_amd.create_model("dedeit", num_classes=C, depth=1)
    assert m.patch_embed.img_size == (224, 224) and tuple(m.pos_embed.shape) == (1, 198, 384) and m.default_cfg["input_size"] == (3, 224, 224)


def test_patch_rows_carries_the_size():
    from devit_amd import ops
    assert ops.IMG_SIZES == SIZES
    pr = ops.PatchRows(None, 5, None, 112)
    assert pr.shape == (5, 3, 112, 112) and pr.grid == 7 and pr.num_patches == 49 and pr.img_size == 112
    pr = ops.PatchRows(None, 2)
    assert pr.shape == (2, 3, 224, 224) and pr.grid == 14 and pr.num_patches == 196
    with pytest.raises(NotImplementedError):
        ops.PatchRows(None, 2, None, 100)


def test_a_batch_of_another_size_is_refused_before_any_launch():
    """ops.expect_side is what VisionTransformer.embed calls first: plain host code, names the model's size and the batch's."""
    from devit_amd import ops
    from devit_amd._lib import DevitError
    assert ops.expect_side(torch.zeros(2, 3, 64, 64), 64, "t") == 64
    with pytest.raises(DevitError, match=r"112 x 112.*64 x 64"):
        ops.expect_side(torch.zeros(2, 3, 64, 64), 112, "t")
    with pytest.raises(DevitError, match=r"224 x 224.*112 x 112"):
        ops.expect_side(ops.PatchRows(None, 2, None, 112), 224, "t")
    for bad in ((2, 3, 100, 100), (2, 3, 64, 48), (2, 1, 64, 64), (2, 3, 240, 240), (3, 64, 64)):
        with pytest.raises(DevitError):
            ops.image_side(torch.zeros(bad), "t")


def test_mix_table_boxes_are_checked_against_the_image_size():
    from devit_amd import ops
    ok = [(2, 0.5, 0, 64, 10, 64), (1, 0.3, 0, 0, 0, 0)]
    assert ops.mix_entries(ok, 64).shape == (2,)
    assert ops.mix_entries([(2, 0.5, 0, 224, 0, 224)]).shape == (1,)                  # the default is 224, as before
    with pytest.raises(ValueError, match="<= 64"):
        ops.mix_entries([(2, 0.5, 0, 65, 0, 10)], 64)
    with pytest.raises(ValueError, match="<= 64"):
        ops.mix_entries([(2, 0.5, 0, 10, 60, 80)], 64)
    with pytest.raises(ValueError):
        ops.mix_table(ok, "cpu", img_size=100)


@pytest.mark.parametrize("mode", ["elem", "pair"])
def test_draw_table_draws_boxes_inside_the_image(mode):
    from devit_amd import ops
    from distill_sub import Mixup
    np.random.seed(3)
    mx = Mixup(0.8, 1.0, 1.0, 0.5, 0.1, 10, mode=mode)
    cut = 0
    for _ in range(20):
        tab = mx.draw_table(8, 64, 64)
        assert ops.mix_entries(tab, 64).tobytes() == tab.tobytes()
        cut += int((tab["mode"] == 2).sum())
        assert int(tab["y1"].max()) <= 64 and int(tab["x1"].max()) <= 64
    assert cut > 10


# ------------------------------------------------------------------------------------------ checkpoints
def test_resize_pos_embed_vs_reference_golden(golden):
    """Within 64 * 2^-24 * max|v|: bicubic is 16 terms with sum |w| < 2 per output, in fp32, doubled for slack -- it absorbs any difference
    between CPU builds of torch.  Token rows are kept as they are."""
    from devit_amd import de_vit
    g = golden("imgsize_resize")
    pe = IM.pos_embed_input()
    bar = 64 * 2.0 ** -24 * float(pe.abs().max())
    for key, G in (("to7", 7), ("to3", 3)):
        got = de_vit.resize_pos_embed(pe, torch.zeros(1, G * G + 2, 64), 2, (G, G))
        assert tuple(got.shape) == (1, G * G + 2, 64) and got.dtype == torch.float32
        assert torch.equal(got[:, :2], pe[:, :2])
        assert float(np.abs(got.numpy() - g[key]).max()) <= bar
        again = de_vit.resize_pos_embed(pe, torch.zeros(1, G * G + 2, 64), 2)          # the grid from the target's shape
        assert torch.equal(again, got)


def test_224_checkpoint_loads_into_a_112_model(tmp_path):
    import devit_amd
    from devit_amd import de_vit
    st = O.make_state(GS, C, "S")
    torch.save({"model": st}, tmp_path / "s224.pth")
    m = devit_amd.create_model("dedeit", pretrained=True, pretrained_path=str(tmp_path / "s224.pth"), num_classes=C, img_size=112)
    want = de_vit.resize_pos_embed(st["pos_embed"], torch.zeros(1, 51, 384), 2, (7, 7))
    sd = m.state_dict()
    assert tuple(sd["pos_embed"].shape) == (1, 51, 384) and torch.equal(sd["pos_embed"], want)
    assert torch.equal(sd["pos_embed"][:, :2], st["pos_embed"][:, :2])
    assert list(sd) == list(st) and all(torch.equal(sd[k], st[k]) for k in st if k != "pos_embed")
    # checkpoint_filter_fn: a flat patch projection is reshaped, everything else passes through, in the checkpoint's order
    flat = dict(st)
    flat["patch_embed.proj.weight"] = st["patch_embed.proj.weight"].reshape(384, 768)
    out = de_vit.checkpoint_filter_fn({"model": flat}, m)
    assert list(out) == list(st) and torch.equal(out["patch_embed.proj.weight"], st["patch_embed.proj.weight"]) and torch.equal(out["pos_embed"], want)
    # a checkpoint of the model's own size is loaded as it is
    m224 = devit_amd.create_model("dedeit", pretrained=True, pretrained_path=str(tmp_path / "s224.pth"), num_classes=C)
    assert torch.equal(m224.state_dict()["pos_embed"], st["pos_embed"])


# ------------------------------------------------------------------------------------------ CLIs
class _Stop(Exception):
    pass


def _sizes_built(monkeypatch):
    """Record the img_size of every PatchEmbed (every model) a CLI's main() builds."""
    from devit_amd import de_vit
    seen, real = [], de_vit.PatchEmbed.__init__

    def init(self, img_size=224, *a, **k):
        seen.append(img_size)
        real(self, img_size, *a, **k)
    monkeypatch.setattr(de_vit.PatchEmbed, "__init__", init)
    return seen


def _stop(*a, **k):
    raise _Stop()


COMMON = ["--synthetic", "1", "--batch-size", "2", "--device", "cpu", "--model", "dedeit", "--teacher-model", "devit", "--epochs", "1"]


@pytest.mark.parametrize("size", [64, 224, None])
def test_distill_sub_and_train_subdata_build_their_models_at_input_size(monkeypatch, tmp_path, size):
    import distill_sub
    import train_subdata
    from devit_amd import ddp
    flag = [] if size is None else ["--input-size", str(size)]
    want = size or 224
    monkeypatch.setattr(ddp, "FlatParams", _stop)              # main() has built student and teacher when it gets here
    for mod, extra in ((distill_sub, []), (train_subdata, ["--distillation-type", "hard"])):
        seen = _sizes_built(monkeypatch)
        args = argparse.ArgumentParser(parents=[mod.get_args_parser()]).parse_args(COMMON + flag + extra + ["--output_dir", str(tmp_path)])
        assert args.input_size == want
        with pytest.raises(_Stop):
            mod.main(args)
        assert seen == [want, want], (mod.__name__, seen)
    loader = distill_sub.SyntheticLoader(1, 2, 5, "cpu", 0, want)
    assert next(iter(loader))[0].shape == (2, 3, want, want)


def test_ensemble_and_shrink_build_their_models_at_input_size(monkeypatch, tmp_path):
    import ensemble
    import shrink
    from devit_amd import engine
    from devit_amd import shrink as shrink_ops
    seen = _sizes_built(monkeypatch)
    monkeypatch.setattr(engine, "evaluate_ens_disjoint", _stop)           # --eval: main() has built its models when it gets to either
    monkeypatch.setattr(shrink_ops, "compact", _stop)
    args = argparse.ArgumentParser(parents=[ensemble.get_args_parser()], conflict_handler="resolve").parse_args(
        COMMON + ["--input-size", "48", "--eval", "--sub_classes", "5", "5", "--output_dir", str(tmp_path)])
    with pytest.raises(_Stop):
        ensemble.main(args)
    assert seen == [48, 48, 48]                                  # the teacher and two backbones
    seen = _sizes_built(monkeypatch)
    monkeypatch.setattr(shrink_ops, "model_geometry", _stop)
    args = argparse.ArgumentParser(parents=[shrink.get_args_parser()]).parse_args(
        ["--synthetic", "1", "--batch-size", "2", "--device", "cpu", "--input-size", "96", "--output_dir", str(tmp_path)])
    with pytest.raises(_Stop):
        shrink.main(args)
    assert seen == [96]


@pytest.mark.parametrize("cli", ["distill_sub", "train_subdata", "ensemble", "shrink"])
def test_unsupported_input_size_exits_with_the_list(cli, tmp_path):
    import importlib
    mod = importlib.import_module(cli)
    base = ["--synthetic", "1", "--batch-size", "2", "--device", "cpu", "--output_dir", str(tmp_path)]
    for bad in ("100", "240", "16"):
        args = argparse.ArgumentParser(parents=[mod.get_args_parser()], conflict_handler="resolve").parse_args(base + ["--input-size", bad])
        with pytest.raises(SystemExit) as e:
            mod.main(args)
        assert "--input-size " + bad in str(e.value) and str(list(SIZES)) in str(e.value)


# ------------------------------------------------------------------------------------------ accounting
def test_flops_at_another_size_differ_in_the_patch_term_and_the_token_count_only():
    from devit_amd import flops as F
    assert abs(F.forward_gflops(emb=384, head=6) - 9.197764608) < 1e-9 and abs(F.forward_gflops() - 35.127656448) < 1e-9      # 224: unchanged
    assert F.forward_gflops(emb=384, head=6, img_size=224, seq_length=197) == F.forward_gflops(emb=384, head=6)
    assert abs(F.step_gflops_per_image() - 63.503) < 1e-3
    assert F.seq_length_for(224, 1) == 197 and F.seq_length_for(224, 2) == 198 and F.seq_length_for(112, 2) == 51 and F.seq_length_for(160, 2) == 102
    for S in (32, 112, 160):
        N = F.seq_length_for(S, 1)
        for kw in (dict(emb=384, head=6), dict(emb=768, head=12, neuron_sparsity=[0.3] * 12, head_sparsity=[0.3] * 12)):
            a = F.forward_gflops(seq_length=N, img_size=S, **kw)
            # the same token count at 224: exactly the patch term differs
            b = F.forward_gflops(seq_length=N, **kw)
            assert abs((b - a) * 1e9 - 2 * 3 * kw["emb"] * (224 ** 2 - S ** 2)) < 1e-3
            assert a < F.forward_gflops(**kw)
        assert F.params_m(emb=384, head=6, seq_length=N, img_size=S) == F.params_m(emb=384, head=6, seq_length=N)
        assert abs((F.params_m(emb=384, head=6) - F.params_m(emb=384, head=6, seq_length=N)) * 1e6 - (197 - N) * 384) < 1e-3
    assert F.relation_loss_gflop() == F.RELATION_LOSS_GFLOP and abs(F.relation_loss_gflop(51) - F.RELATION_LOSS_GFLOP * (51 / 198) ** 2) < 1e-12
    t = F.seq_length_for(112, 2)
    assert F.step_gflops_per_image(25, t, 112) < 0.3 * F.step_gflops_per_image()
    assert F.step_gflops_per_image_executed(25, t, 112) < F.step_gflops_per_image(25, t, 112)


def test_shrink_accounting_uses_the_model_s_size():
    import devit_amd
    from devit_amd import flops as F
    from devit_amd import shrink
    m224 = devit_amd.create_model("dedeit", num_classes=C)
    m112 = devit_amd.create_model("dedeit", num_classes=C, img_size=112)
    assert shrink.model_geometry(m224) == dict(emb=384, head=6, layer=12, mlp_ratio=4)                      # as before
    geo = shrink.model_geometry(m112)
    assert geo == dict(emb=384, head=6, layer=12, mlp_ratio=4, img_size=112, seq_length=50)
    assert shrink.macs_target(0.3, **geo) == 0.3 * F.forward_gflops(emb=384, head=6, seq_length=50, img_size=112)
    x = np.random.default_rng(0).uniform(0, 0.5, size=(4, 24))
    rows = shrink._macs_g_rows(x, **geo)
    for r, got in zip(x, rows):
        assert got == F.macs_g(neuron_sparsity=r[:12], head_sparsity=r[12:], **geo)
    assert abs(shrink.compacted_gflops(m224, num_classes=C) - shrink.compacted_gflops(m224, tokens=198, num_classes=C)) == 0
    assert abs(shrink.compacted_gflops(m112, num_classes=C) - shrink.compacted_gflops(m112, tokens=51, num_classes=C)) == 0
    assert shrink.compacted_gflops(m112, num_classes=C) < 0.3 * shrink.compacted_gflops(m224, num_classes=C)
