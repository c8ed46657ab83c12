"""Host logic of the optimizer tails, no GPU: the factory that maps the command line to a class, the support check of the three training CLIs,
FlatLamb's chunk table over a CPU ddp.FlatParams of dedeit and its validation, the state dicts with their kind check, and the C calls of one
FlatAdamW.step in their order."""
import importlib

import pytest
import torch

import devit_amd
from devit_amd import _lib, ddp, optim


@pytest.fixture(scope="module")
def small():
    torch.manual_seed(0)
    model = devit_amd.create_model("dedeit", depth=2, num_classes=25)
    return model, ddp.FlatParams(model)


def _args(cli="distill_sub", *argv):
    mod = importlib.import_module(cli)
    args, _ = mod.get_args_parser().parse_known_args(list(argv))
    return args


@pytest.mark.parametrize("name,cls", [("adamw", "FlatAdamW"), ("adam", "FlatAdam"), ("momentum", "FlatSGD"), ("nesterov", "FlatSGD"),
                                      ("lamb", "FlatLamb"), ("lambc", "FlatLamb"), ("LAMB", "FlatLamb")])
def test_factory_maps_the_command_line(small, name, cls):
    model, flat = small
    args = _args("distill_sub", "--opt", name, "--momentum", "0.8", "--opt-eps", "1e-6", "--opt-betas", "0.8", "0.95", "--weight-decay", "0.05",
                 "--clip-grad", "2.0", "--model-ema-decay", "0.99")
    opt = optim.create_flat_optimizer(args, flat, model)
    assert type(opt).__name__ == cls and opt.flat is flat
    assert opt.param_groups[0]["lr"] == args.lr and opt.max_norm == 2.0 and opt.weight_decay == 0.05 and opt.ema_decay == 0.99
    assert opt.ema is not None and opt.no_decay4 is not None
    if cls == "FlatSGD":
        assert opt.momentum == 0.8 and opt.nesterov == (name == "nesterov") and opt.opt_name == name
    else:
        assert opt.eps == 1e-6 and tuple(opt.betas) == (0.8, 0.95)
    if cls == "FlatLamb":
        assert opt.trust_clip == (name.lower() == "lambc") and opt.opt_name == name.lower()
    no_ema = optim.create_flat_optimizer(_args("distill_sub", "--opt", name, "--no-model-ema"), flat, model)
    assert no_ema.ema is None and no_ema.ema_state_dict(model) is None and tuple(getattr(no_ema, "betas", (0.9, 0.999))) == (0.9, 0.999)
    with pytest.raises(ValueError):
        optim.create_flat_optimizer(_args("distill_sub", "--opt", "rmsprop"), flat, model)


@pytest.mark.parametrize("cli", ["distill_sub", "train_subdata", "ensemble"])
def test_support_check(cli):
    import distill_sub
    for name in ("adamw", "adam", "momentum", "nesterov", "lamb", "lambc", "Nesterov", "LAMBC"):
        distill_sub.check_supported(_args(cli, "--opt", name))
    with pytest.raises(SystemExit, match="use nesterov: timm's sgd is Nesterov SGD"):
        distill_sub.check_supported(_args(cli, "--opt", "sgd"))
    with pytest.raises(SystemExit, match="rmsprop"):
        distill_sub.check_supported(_args(cli, "--opt", "rmsprop"))
    src = open(importlib.import_module(cli).__file__).read()
    assert "create_flat_optimizer" in src and "optim.FlatAdamW(" not in src          # every optimizer of the CLI comes from the factory


def test_ensemble_torch_optim_is_adamw_only():
    import distill_sub
    distill_sub.check_supported(_args("ensemble", "--torch-optim"))
    with pytest.raises(SystemExit, match="torch-optim"):
        distill_sub.check_supported(_args("ensemble", "--torch-optim", "--opt", "lamb"))


def test_lamb_chunk_table(small):
    model, flat = small
    no_decay = optim.no_decay_names(model)
    opt = optim.FlatLamb(flat, weight_decay=0.05, no_decay=no_decay)
    t = opt.chunks_host
    assert t.dtype == torch.int32 and t.shape == (opt.nchunks, 4) and opt.nsegments == len(flat.names)
    assert _lib.load().devit_abi_struct_size(11) == 16 == t.shape[1] * t.element_size()
    owner = torch.full((flat.numel // 4,), -1, dtype=torch.int64)          # granule -> tensor index; -1: padding
    for s, (p, o) in enumerate(zip(flat.params, flat.offsets)):
        assert o % 4 == 0 and bool((owner[o // 4:(o + p.numel() + 3) // 4] == -1).all())
        owner[o // 4:(o + p.numel() + 3) // 4] = s
    hits = torch.zeros_like(owner)
    for first, count, seg, flags in t.tolist():
        assert 1 <= count <= _lib.OPT_CHUNK_GRANULES
        assert bool((owner[first:first + count] == seg).all()), "every chunk lies inside one tensor"
        assert flags == (1 if flat.names[seg] in no_decay else 0), flat.names[seg]
        hits[first:first + count] += 1
    assert bool((hits[owner >= 0] == 1).all()), "every granule of every tensor is covered once (the chunks are disjoint)"
    assert bool((hits[owner < 0] == 0).all()) and int((owner < 0).sum()) > 0, "padding is covered by none"
    assert t[:, 2].tolist() == sorted(t[:, 2].tolist())
    big = flat.names.index("blocks.0.mlp.fc1.weight")
    assert int((t[:, 2] == big).sum()) == (384 * 1536 // 4 + 1023) // 1024 and {f for *_, s, f in t.tolist() if s == big} == {0}
    assert {f for *_, s, f in t.tolist() if s == flat.names.index("head.bias")} == {1}          # 25 elements: seven granules, the last one padded
    # without weight decay timm has one group and Lamb adapts nothing: every tensor is in the no-decay group
    assert bool((optim.FlatLamb(flat, weight_decay=0.0, no_decay=no_decay).chunks_host[:, 3] == 1).all())


def test_chunk_table_validation(small):
    _, flat = small
    sizes = [p.numel() for p in flat.params]
    good = optim.lamb_chunk_table(flat.names, sizes, flat.offsets, set())
    check = lambda t: optim.validate_chunk_table(t, sizes, flat.offsets, flat.numel)
    check(good)

    def broken(row, col, value):
        t = good.clone()
        t[row, col] = value
        return t
    last = good.shape[0] - 1
    two = int((good[1:, 2] == good[:-1, 2]).nonzero()[0])          # the first chunk of a tensor that has more than one
    for what, t in [("out of range", broken(last, 0, flat.numel // 4)), ("too long", broken(0, 1, 1025)), ("empty", broken(0, 1, 0)),
                    ("overlap", broken(1, 0, int(good[0, 0]))), ("straddles two tensors", broken(0, 1, int(good[0, 1]) + 1)),
                    ("hole", torch.cat([good[:3], good[4:]])), ("unknown tensor", broken(last, 2, len(sizes))),
                    ("unsorted", torch.cat([good[1:], good[:1]])), ("of mixed flags within a tensor", broken(two, 3, 1))]:
        with pytest.raises(ValueError):
            check(t)
            pytest.fail(f"a chunk table that is {what} passed the validation")


@pytest.mark.parametrize("make", [lambda f: optim.FlatSGD(f, nesterov=True, ema_decay=0.9), lambda f: optim.FlatAdam(f, ema_decay=0.9),
                                  lambda f: optim.FlatLamb(f, weight_decay=0.05, ema_decay=0.9, trust_clip=True)],
                         ids=["nesterov", "adam", "lambc"])
def test_state_dict_round_trip(small, make):
    _, flat = small
    a, b = make(flat), make(flat)
    g = torch.Generator().manual_seed(1)
    for k in a.state_keys:
        getattr(a, k).copy_(torch.randn(flat.numel, generator=g))
    a.ema.copy_(torch.randn(flat.numel, generator=g))
    a.step_count, a.param_groups[0]["lr"] = 17, 0.125
    sd = a.state_dict()
    assert sd["opt"] == a.opt_name and set(sd) == {"opt", "ema", "step", "lr", *a.state_keys}
    b.load_state_dict(sd)
    assert b.step_count == 17 and b.param_groups[0]["lr"] == 0.125 and torch.equal(b.ema, a.ema)
    assert all(torch.equal(getattr(a, k), getattr(b, k)) for k in a.state_keys)


def test_state_dict_of_another_kind_is_refused(small):
    _, flat = small
    kinds = {"adamw": optim.FlatAdamW(flat), "adam": optim.FlatAdam(flat), "momentum": optim.FlatSGD(flat), "nesterov": optim.FlatSGD(flat, nesterov=True),
             "lamb": optim.FlatLamb(flat), "lambc": optim.FlatLamb(flat, trust_clip=True)}
    assert set(optim.FlatAdamW(flat).state_dict()) == {"m", "v", "ema", "step", "lr"}          # FlatAdamW's checkpoints keep their keys
    for src, a in kinds.items():
        for dst, b in kinds.items():
            if src == dst:
                b.load_state_dict(a.state_dict())
                continue
            with pytest.raises(ValueError) as e:
                b.load_state_dict(a.state_dict())
            assert src in str(e.value) and dst in str(e.value)


def test_adamw_step_host_sequence(small, monkeypatch):
    """the C calls of FlatAdamW.step: the norm only when the step clips, then exactly one devit_adamw_step that finds lr and the two bias
    corrections of ITS step in `dyn`; the device check comes first, grad_scale is consumed once"""
    _, flat = small
    log = []
    monkeypatch.setattr(_lib, "require_device", lambda t: log.append(("require_device", None)))
    monkeypatch.setattr(optim, "stream_ptr", lambda: None)
    for max_norm in (None, 0.0, 2.0):
        opt = optim.FlatAdamW(flat, lr=0.25, betas=(0.5, 0.75), max_norm=max_norm)
        monkeypatch.setattr(optim, "call", lambda name, *a: log.append((name, (opt.step_count, opt._dyn.tolist(), flat.grad_scale, a))))
        for t in (1, 2):
            del log[:]
            flat.grad_scale = 0.5
            opt.param_groups[0]["lr"] = 0.25 / t
            opt.step()
            assert [n for n, _ in log] == ["require_device"] + (["devit_sumsq_f32"] if max_norm else []) + ["devit_adamw_step"]
            count, dyn, scale, args = log[-1][1]
            assert count == t and dyn == [0.25 / t, 1 - 0.5 ** t, 1 - 0.75 ** t]          # all exact in fp32
            assert scale == 0.5 and args[16] == 0.5 and flat.grad_scale == 1.0
            assert (args[7] is None) == (not max_norm) and args[9] == flat.numel and args[10:13] == (0.5, 0.75, opt.eps)
