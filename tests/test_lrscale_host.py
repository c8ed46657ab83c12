"""Host logic of layer-wise learning-rate decay (`--layer-decay`), no GPU: the layer ids and scales of the models the CLIs
train, written out from the definition (stem 0, blocks.<i> i + 1, the rest depth + 1; scale = decay^(depth + 1 - id) in float64, stored as fp32);
the group bytes and the 256-entry table over a flat buffer; what _FlatTail._setup refuses; the parser, the CLIs' refusals, the factory, the
state dict's key and its mismatch error; and the C call each tail's step makes."""
import importlib
import math

import pytest
import torch

import devit_amd
from devit_amd import _lib, ddp, optim
from devit_amd.ensemble_models import EnsMLP, MultiViT


def _names(model):
    return [n for n, _ in model.named_parameters()]


def _meta(make):
    return make()          # (only the names are read; the constructors draw a scalar per block, which no meta device gives)


def f32(x):
    return float(torch.tensor(x, dtype=torch.float64).to(torch.float32))


# ------------------------------------------------------------------------------------------ ids and scales
@pytest.mark.parametrize("model,depth,distilled", [("dedeit", 12, True), ("deit_base_distilled_patch16_224", 12, True), ("devit", 12, False),
                                                   ("vit_large_patch16_224", 24, False)])
def test_layer_ids_and_scales(model, depth, distilled):
    names = _names(_meta(lambda: devit_amd.create_model(model, num_classes=10)))
    ids = optim.layer_ids(names, depth)
    assert set(ids) == set(names) and set(ids.values()) == set(range(depth + 2))          # vit_large: 26 groups
    assert ids["cls_token"] == ids["pos_embed"] == ids["patch_embed.proj.weight"] == ids["patch_embed.proj.bias"] == 0
    assert ("dist_token" in ids) == distilled and ("head_dist.weight" in ids) == distilled
    if distilled:
        assert ids["dist_token"] == 0 and ids["head_dist.weight"] == ids["head_dist.bias"] == depth + 1
    assert ids["norm.weight"] == ids["norm.bias"] == ids["head.weight"] == ids["head.bias"] == depth + 1
    per_block = [n[len("blocks.0."):] for n in names if n.startswith("blocks.0.")]
    assert len(per_block) == 12
    for i in range(depth):
        assert all(ids[f"blocks.{i}.{t}"] == i + 1 for t in per_block)
    assert len(names) == 12 * depth + (4 if not distilled else 5) + 4 + (2 if distilled else 0)
    decay = 0.75
    scales = optim.layer_decay_scales(names, depth, decay)
    assert scales["head.weight"] == scales["norm.bias"] == 1.0
    assert scales[f"blocks.{depth - 1}.mlp.fc2.weight"] == 0.75 and scales[f"blocks.{depth - 2}.attn.qkv.bias"] == 0.5625
    assert scales["blocks.0.norm1.weight"] == f32(0.75 ** depth) and scales["pos_embed"] == scales["cls_token"] == f32(0.75 ** (depth + 1))
    assert len(set(scales.values())) == depth + 2
    assert all(v == f32(decay ** (depth + 1 - ids[n])) for n, v in scales.items())


def test_layer_ids_ignore_a_prefix():
    multi = _meta(lambda: MultiViT("dedeit", num_classes_list=[5, 5], num_div=2))
    names = _names(multi)
    assert optim.model_depth(multi) == 12
    ids = optim.layer_ids(names, 12)
    for k in (0, 1):
        assert ids[f"backbones.{k}.cls_token"] == ids[f"backbones.{k}.dist_token"] == ids[f"backbones.{k}.pos_embed"] == 0
        assert ids[f"backbones.{k}.patch_embed.proj.weight"] == 0 and ids[f"backbones.{k}.norm.weight"] == 13
        assert ids[f"backbones.{k}.blocks.0.attn.qkv.weight"] == 1 and ids[f"backbones.{k}.blocks.11.mlp.fc2.bias"] == 12
    assert not any(".head" in n for n in names)          # MultiViT's backbones have no classifier
    assert set(ids.values()) == set(range(14))
    plain = optim.layer_ids(["module.blocks.3.norm1.weight", "module.pos_embed", "module.head.bias", "resize_mlp.weight", "module.resize_att_mlp.bias"], 12)
    assert list(plain.values()) == [4, 0, 13, 13, 13]
    assert optim.layer_ids(["my_blocks.3.x", "xblocks.3.y", "not_pos_embed", "pos_embed.extra"], 12) == \
        {"my_blocks.3.x": 13, "xblocks.3.y": 13, "not_pos_embed": 13, "pos_embed.extra": 13}          # whole path components only
    with pytest.raises(ValueError, match="depth 2"):
        optim.layer_ids(["blocks.2.norm1.weight"], 2)
    with pytest.raises(ValueError):
        optim.model_depth(EnsMLP("dedeit", 10, 384, [5, 5], 768))


# ------------------------------------------------------------------------------------------ the byte array and the table
@pytest.fixture(scope="module")
def small():
    torch.manual_seed(0)
    model = devit_amd.create_model("dedeit", depth=2, num_classes=25)
    return model, ddp.FlatParams(model)


def _owner(flat):
    owner = torch.full((flat.numel // 4,), -1, dtype=torch.int64)          # granule -> tensor index; -1: padding
    for s, (p, o) in enumerate(zip(flat.params, flat.offsets)):
        owner[o // 4:(o + p.numel() + 3) // 4] = s
    return owner


def test_group_bytes_and_table(small):
    model, flat = small
    scales = optim.layer_decay_scales(flat.names, 2, 0.5)
    opt = optim.FlatAdamW(flat, lr_scales=scales)
    g4, table = opt.lr_group4, opt.lr_scales
    assert g4.dtype == torch.uint8 and g4.shape == (flat.numel // 4,) and table.dtype == torch.float32 and table.shape == (256,)
    assert table[:4].tolist() == [1.0, 0.125, 0.25, 0.5] and bool((table[4:] == 1.0).all())          # scale 1 first, then ascending; unused entries 1
    owner = _owner(flat)
    assert int((owner < 0).sum()) > 0 and bool((g4[owner < 0] == 0).all()) and float(table[0]) == 1.0, "padding carries the group of scale 1"
    for s, name in enumerate(flat.names):
        mine = g4[owner == s]
        assert mine.numel() == (flat.params[s].numel() + 3) // 4 and bool((table[mine.long()] == scales[name]).all()), name
    hb = flat.names.index("head.bias")
    assert flat.params[hb].numel() == 25 and int((owner == hb).sum()) == 7, "25 elements: seven granules, the last one partial"
    assert float(table[int(g4[owner == flat.names.index("patch_embed.proj.weight")][0])]) == 0.125          # decay^(depth + 1)
    # a partial dict: tensors it does not name train at the scheduled lr; a scale of 0 is allowed
    opt = optim.FlatSGD(flat, lr_scales={"pos_embed": 0.0, "head.weight": 3.0})
    assert opt.lr_scales[:3].tolist() == [1.0, 0.0, 3.0]
    assert sorted(set(opt.lr_group4[owner == flat.names.index("pos_embed")].tolist())) == [1]
    assert int((opt.lr_group4 != 0).sum()) == int((owner == flat.names.index("pos_embed")).sum()) + int((owner == flat.names.index("head.weight")).sum())
    assert optim.FlatAdam(flat).lr_scales is None and optim.FlatAdam(flat).lr_group4 is None


def test_setup_refuses(small):
    _, flat = small
    for bad in (-0.5, math.nan, math.inf, -math.inf):
        with pytest.raises(ValueError, match="finite and >= 0"):
            optim.FlatAdamW(flat, lr_scales={"head.weight": bad})
    with pytest.raises(ValueError, match="head.wait"):
        optim.FlatLamb(flat, lr_scales={"head.wait": 0.5})
    names = [f"t{i}" for i in range(300)]
    sizes, offsets = [4] * 300, [4 * i for i in range(300)]
    ok = {n: 1.0 - i / 512 for i, n in enumerate(names[:256])}          # 256 distinct scales, 1.0 among them
    g4, table = optim.lr_scale_table(names, sizes, offsets, 1280, ok)
    assert sorted(set(g4[:256].tolist())) == list(range(256)) and bool((g4[256:] == 0).all()) and 255 in g4.tolist()
    assert all(float(table[int(g4[i])]) == f32(ok[names[i]]) for i in range(256))
    with pytest.raises(ValueError, match="257 distinct"):
        optim.lr_scale_table(names, sizes, offsets, 1280, dict(ok, t256=0.25 / 512))
    # scales that differ in float64 and agree in fp32 are one group
    g4, table = optim.lr_scale_table(names, sizes, offsets, 1280, {"t0": 0.1, "t1": float(torch.tensor(0.1, dtype=torch.float32))})
    assert g4[:2].tolist() == [1, 1]


# ------------------------------------------------------------------------------------------ the CLIs and the factory
def _args(cli="distill_sub", *argv):
    mod = importlib.import_module(cli)
    args, _ = mod.get_args_parser().parse_known_args(list(argv))
    return args


@pytest.mark.parametrize("cli", ["distill_sub", "train_subdata", "ensemble"])
def test_parser_and_refusals(cli):
    import distill_sub
    assert _args(cli).layer_decay is None
    assert _args(cli, "--layer-decay", "0.75").layer_decay == 0.75
    for ok in ("0.75", "1.0", "1e-3"):
        distill_sub.check_supported(_args(cli, "--layer-decay", ok))
    for bad in ("0", "-0.5", "1.01", "nan", "inf"):
        with pytest.raises(SystemExit, match="layer-decay"):
            distill_sub.check_supported(_args(cli, "--layer-decay", bad))


def test_ensemble_torch_optim_refuses_layer_decay():
    import distill_sub
    with pytest.raises(SystemExit, match="torch-optim --layer-decay 0.75: the per-layer learning rates live in the fused tails"):
        distill_sub.check_supported(_args("ensemble", "--torch-optim", "--layer-decay", "0.75"))
    src = open(importlib.import_module("ensemble").__file__).read()
    assert "create_flat_optimizer(args, ens_flat, ens_model, layer_decay=False)" in src          # the fusion head's optimizer stays unscaled


@pytest.mark.parametrize("name", ["adamw", "adam", "nesterov", "lamb"])
def test_factory_and_state_dict(small, name, capsys):
    model, flat = small
    plain = optim.create_flat_optimizer(_args("distill_sub", "--opt", name), flat, model)
    one = optim.create_flat_optimizer(_args("distill_sub", "--opt", name, "--layer-decay", "1.0"), flat, model)
    capsys.readouterr()
    opt = optim.create_flat_optimizer(_args("distill_sub", "--opt", name, "--layer-decay", "0.5"), flat, model)
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("--layer-decay 0.5: layer")]
    assert len(lines) == 4 and [int(l.split()[-2]) for l in lines] == [5, 12, 12, 6], lines          # one line per id: id, scale, tensor count
    assert "0.125" in lines[0] and "lr x 1 " in lines[3]
    for o in (plain, one):          # 1.0 is the unscaled path
        assert o.lr_scales is None and o.lr_group4 is None and o.layer_decay is None and "layer_decay" not in o.state_dict()
    assert set(plain.state_dict()) == {"ema", "step", "lr", *plain.state_keys} | ({"opt"} if name != "adamw" else set())
    assert opt.layer_decay == 0.5 and opt.lr_scales.shape == (256,) and opt.lr_scales[:4].tolist() == [1.0, 0.125, 0.25, 0.5]
    sd = opt.state_dict()
    assert sd["layer_decay"] == 0.5 and set(sd) == set(plain.state_dict()) | {"layer_decay"}
    assert not any(torch.is_tensor(v) and v.shape == (256,) for v in sd.values()), "the scales are rebuilt from the flag, not stored"
    opt.load_state_dict(sd)
    other = optim.create_flat_optimizer(_args("distill_sub", "--opt", name, "--layer-decay", "0.75"), flat, model)
    for src, dst, a, b in ((sd, other, "0.5", "0.75"), (sd, plain, "0.5", "None"), (plain.state_dict(), opt, "None", "0.5")):
        with pytest.raises(ValueError, match=f"--layer-decay {a} cannot be loaded into --layer-decay {b}"):
            dst.load_state_dict(src)
    # the ensemble's fusion head: the flag is not read
    ens = EnsMLP("dedeit", 10, 384, [5, 5], 768)
    head = optim.create_flat_optimizer(_args("ensemble", "--opt", name, "--layer-decay", "0.5"), ddp.FlatParams(ens), ens, layer_decay=False)
    assert head.lr_scales is None and "layer_decay" not in head.state_dict()
    multi = MultiViT("dedeit", drop_path=0.0, num_classes_list=[5, 5], num_div=2)
    mflat = ddp.FlatParams(multi)
    mopt = optim.create_flat_optimizer(_args("ensemble", "--opt", name, "--layer-decay", "0.5"), mflat, multi)
    assert mopt.layer_decay == 0.5 and float(mopt.lr_scales[1]) == 0.5 ** 13 and len(set(mopt.lr_group4.tolist())) == 14


@pytest.mark.parametrize("kind", ["adamw", "adam", "momentum", "lamb"])
def test_step_calls_the_lrs_entry_point(small, monkeypatch, kind):
    """with a table the step's one C call is the *_lrs entry point, the sibling's arguments followed by the two arrays and the stream; without one
    it is the sibling, as before"""
    _, flat = small
    make = {"adamw": optim.FlatAdamW, "adam": optim.FlatAdam, "momentum": optim.FlatSGD, "lamb": optim.FlatLamb}[kind]
    entry = {"adamw": "devit_adamw_step", "adam": "devit_adam_l2_step", "momentum": "devit_sgd_step", "lamb": "devit_lamb_step"}[kind]
    log = []
    monkeypatch.setattr(_lib, "require_device", lambda t: None)
    monkeypatch.setattr(optim, "stream_ptr", lambda: "stream")
    monkeypatch.setattr(optim, "call", lambda name, *a: log.append((name, a)))
    plain, scaled = make(flat, max_norm=1.0), make(flat, max_norm=1.0, lr_scales={"head.weight": 0.5})
    plain.step()
    scaled.step()
    assert [n for n, _ in log] == ["devit_sumsq_f32", entry, "devit_sumsq_f32", entry + "_lrs"]
    a, b = log[1][1], log[3][1]
    assert len(a) == len(_lib.SIGNATURES[entry][1]) and len(b) == len(_lib.SIGNATURES[entry + "_lrs"][1]) == len(a) + 2
    assert [b[-3].value, b[-2].value] == [scaled.lr_group4.data_ptr(), scaled.lr_scales.data_ptr()] and b[-1] == a[-1] == "stream"
    assert _lib.SIGNATURES[entry + "_lrs"][1][:len(a) - 1] == _lib.SIGNATURES[entry][1][:-1]
