"""The optimizer of csrc/optim.hip on a real MI355X against the float64 statements of tests/_optim_model.py, on the inputs tests/test_optim_model.py
holds the model itself to: devit_sumsq_f32, then devit_adamw_step, devit_sgd_step (momentum, nesterov), devit_adam_l2_step and devit_lamb_step (lamb, lambc) at the kernel level -- three chained
steps, each held element by element against the statement applied to the fp32 state the kernel itself left behind, the bf16 copy bit-exact, guard
elements behind every buffer -- then FlatSGD / FlatAdam / FlatLamb behind one real backward of a two-block dedeit, and the CLIs with --opt."""
import argparse
import json
import os

import pytest
import torch

import _optim_model as M
import _tail_model as T
from _tail_model import BF16, F32, F64, ratio
from conftest import chk
from test_gpu_tail import Out, call, hold, refused, same_bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from devit_amd import _lib
    _lib.require_device(torch.zeros(1, device="cuda"))
    return torch.device("cuda")


def _L():
    from devit_amd import _lib
    return _lib


def _report(tag, worst):
    for k, r in worst.items():
        print(f"tail/{tag}/{k} {r:.3f}")
        assert chk(r, 1.0, name=f"tail/{tag}/{k}"), (tag, k, r)


def _cid(c):
    return f"n{c['n']}-mn{c['max_norm']}-gs{c['grad_scale']}-gn{int(c['gnorm'])}-e{int(c['ema'])}"


# ============================================================================================ devit_sumsq_f32, devit_adamw_step
@pytest.mark.parametrize("n", M.SUMSQ_NS)
def test_sumsq_f32(dev, n):
    L = _L()
    nws = L.load().devit_sumsq_workspace()
    for ints in (True, False):
        gv = M.sumsq_inputs(n, ints)
        ref, bnd = M.sumsq_bounds(gv)
        out, ws = Out(dev, 1, 1), Out(dev, 1, nws // 4)
        call("devit_sumsq_f32", gv.to(dev), n, out.t, ws.t, nws)
        assert out.intact() and ws.intact()
        if ints:
            assert float(out.v[0, 0]) == float(ref), "integers in [-2, 2]: every partial sum is exact"
        else:
            hold(f"sumsq_f32/n{n}/out", out.v[0, 0], ref, bnd)


def test_sumsq_f32_refuses_n6(dev):
    t = torch.zeros(1024, device=dev)
    refused("devit_sumsq_f32", t, 6, t, t, 4096)


@pytest.mark.parametrize("c", M.step_cases(), ids=lambda c: f"n{c['n']}-mn{c['max_norm']}-gs{c['grad_scale']}-gn{int(c['gnorm'])}-e{int(c['ema'])}")
def test_adamw_step(dev, c):
    """three chained steps; each is held against the float64 statement applied to the fp32 state the kernel itself left behind"""
    L = _L()
    i = M.step_inputs(c)
    n, hp = c["n"], M.ADAM_HP
    p, m, v = Out(dev, 1, n, init=i["p"]), Out(dev, 1, n, init=torch.zeros(n)), Out(dev, 1, n, init=torch.zeros(n))
    ema = Out(dev, 1, n, init=i["p"]) if c["ema"] else None
    p16 = Out(dev, 1, n, BF16) if c["p16"] else None
    mask = None if i["mask"] is None else i["mask"].to(dev)
    nws = L.load().devit_sumsq_workspace()
    ws, gsq = torch.empty(nws, dtype=torch.uint8, device=dev), torch.empty(1, device=dev)
    tag = f"adamw_step/n{n}_mn{c['max_norm']}_gs{c['grad_scale']}_gn{int(c['gnorm'])}_mask{int(c['mask'])}"
    worst = {}
    for step in (1, 2, 3):
        g = i["grads"][step - 1]
        gd = g.to(dev)
        before = [t.v[0].cpu().clone() if t is not None else None for t in (p, m, v, ema)]
        if c["gnorm"]:
            call("devit_sumsq_f32", gd, n, gsq, ws, nws)
        dyn = torch.tensor([hp["lr"], 1 - hp["beta1"] ** step, 1 - hp["beta2"] ** step], dtype=F32, device=dev)
        call("devit_adamw_step", p.t, gd, m.t, v.t, ema.t if ema else None, p16.t if p16 else None, mask, gsq if c["gnorm"] else None, dyn, n,
             hp["beta1"], hp["beta2"], hp["eps"], hp["wd"], c["max_norm"], hp["ema_decay"], c["grad_scale"])
        ref, bnd = M.adamw_step_bounds(before[0], g, before[1], before[2], before[3], i["mask"], gsq.cpu() if c["gnorm"] else None, step,
                                       c["max_norm"], c["grad_scale"])
        got = dict(p=p, m=m, v=v, ema=ema)
        for k in ref:
            assert got[k].intact()
            worst[k] = max(worst.get(k, 0.0), ratio(got[k].v[0], ref[k], bnd[k]))
        if p16:
            assert p16.intact() and same_bits(p16.v, p.v.to(BF16)), "p_bf16 == bf16(p)"
        if step == 1:
            z = g == 0
            assert bool((m.v[0].cpu()[z] == 0).all()) and bool((v.v[0].cpu()[z] == 0).all()), "a zero gradient leaves zero moments at step 1"
    for k, r in worst.items():
        print(f"tail/{tag}/{k} {r:.3f}")
        assert chk(r, 1.0, name=f"tail/{tag}/{k}"), (tag, k, r)


# ============================================================================================ devit_sgd_step, devit_adam_l2_step
@pytest.mark.parametrize("kind", ["momentum", "nesterov", "adam"])
@pytest.mark.parametrize("c", M.step_cases(), ids=_cid)
def test_sgd_and_adam_steps(dev, c, kind):
    L = _L()
    i = M.step_inputs(c)
    n, hp = c["n"], M.OPT_HP
    names = ("p", "buf") if kind != "adam" else ("p", "m", "v")
    st = {k: Out(dev, 1, n, init=i["p"] if k == "p" else torch.zeros(n)) for k in names}
    if c["ema"]:
        st["ema"] = Out(dev, 1, n, init=i["p"])
    p16 = Out(dev, 1, n, BF16) if c["p16"] else None
    mask = None if i["mask"] is None else i["mask"].to(dev)
    nws = L.load().devit_sumsq_workspace()
    ws, gsq = torch.empty(nws, dtype=torch.uint8, device=dev), torch.empty(1, device=dev)
    worst = {}
    for step in (1, 2, 3):
        g = i["grads"][step - 1]
        gd = g.to(dev)
        before = {k: t.v[0].cpu().clone() for k, t in st.items()}
        if c["gnorm"]:
            call("devit_sumsq_f32", gd, n, gsq, ws, nws)
        ema_t, p16_t, gsq_t = st["ema"].t if c["ema"] else None, p16.t if p16 else None, gsq if c["gnorm"] else None
        tail = (i["mask"], gsq.cpu() if c["gnorm"] else None, step, c["max_norm"], c["grad_scale"])
        if kind == "adam":
            dyn = torch.tensor([hp["lr"], 1 - hp["beta1"] ** step, 1 - hp["beta2"] ** step], dtype=F32, device=dev)
            call("devit_adam_l2_step", st["p"].t, gd, st["m"].t, st["v"].t, ema_t, p16_t, mask, gsq_t, dyn, n, hp["beta1"], hp["beta2"], hp["eps"],
                 hp["wd"], c["max_norm"], hp["ema_decay"], c["grad_scale"])
            ref, bnd = M.adam_step_bounds(before["p"], g, before["m"], before["v"], before.get("ema"), *tail)
        else:
            dyn = torch.tensor([hp["lr"]], dtype=F32, device=dev)
            call("devit_sgd_step", st["p"].t, gd, st["buf"].t, ema_t, p16_t, mask, gsq_t, dyn, n, hp["momentum"], int(kind == "nesterov"),
                 hp["wd"], c["max_norm"], hp["ema_decay"], c["grad_scale"])
            ref, bnd = M.sgd_step_bounds(before["p"], g, before["buf"], before.get("ema"), *tail, kind == "nesterov")
        assert set(ref) == set(st)
        for k in ref:
            assert st[k].intact()
            worst[k] = max(worst.get(k, 0.0), ratio(st[k].v[0], ref[k], bnd[k]))
        if p16:
            assert p16.intact() and same_bits(p16.v, st["p"].v.to(BF16)), "p_bf16 == bf16(p)"
    _report(f"{kind}_step/{_cid(c)}_mask{int(c['mask'])}", worst)


def test_step_refusals(dev):
    t = torch.zeros(1024, device=dev)
    refused("devit_sgd_step", t, t, t, None, None, None, None, t, 6, 0.9, 0, 0.0, 0.0, 0.0, 1.0)
    refused("devit_sgd_step", t, t, None, None, None, None, None, t, 8, 0.9, 0, 0.0, 0.0, 0.0, 1.0)
    refused("devit_adam_l2_step", t, t, t, t, None, None, None, None, t, 6, 0.9, 0.999, 1e-8, 0.0, 0.0, 0.0, 1.0)
    refused("devit_adam_l2_step", t, t, t, None, None, None, None, None, t, 8, 0.9, 0.999, 1e-8, 0.0, 0.0, 0.0, 1.0)
    chunks = torch.tensor([[0, 2, 0, 0]], dtype=torch.int32, device=dev)
    lamb = lambda n, gsq, ch, nch, nseg, ws, nws: ("devit_lamb_step", t, t, t, t, None, None, gsq, t, n, ch, nch, nseg, 0, 0.9, 0.999, 1e-8, 0.0, 0.0, 0.0,
                                                   1.0, ws, nws)
    need = _L().load().devit_lamb_workspace(1, 1)
    assert need == 12
    refused(*lamb(6, t, chunks, 1, 1, t, 4096))
    refused(*lamb(8, None, chunks, 1, 1, t, 4096))          # LAMB clips to norm 1 itself: the norm is required
    refused(*lamb(8, t, None, 1, 1, t, 4096))
    refused(*lamb(8, t, chunks, 0, 1, t, 4096))
    refused(*lamb(8, t, chunks, 1, 0, t, 4096))
    refused(*lamb(8, t, chunks, 1, 1, t, need - 1))
    refused(*lamb(8, t, chunks, 1, 1, None, 4096))


# ============================================================================================ devit_lamb_step
def _lid(c):
    return f"{'lambc' if c['trust_clip'] else 'lamb'}-par{c['exempt_parity']}-mn{c['max_norm']}-gs{c['grad_scale']}"


def _lamb_run(dev, c, i, table):
    """three chained steps from the inputs -> (the outputs' bits after the last step, worst ratios); every step is held against the statement applied to
    the state the kernels left"""
    L = _L()
    n, hp, nseg = i["n"], M.OPT_HP, len(i["layout"])
    st = dict(p=Out(dev, 1, n, init=i["p"]), m=Out(dev, 1, n, init=i["m"]), v=Out(dev, 1, n, init=i["v"]))
    if c["ema"]:
        st["ema"] = Out(dev, 1, n, init=i["p"])
    p16 = Out(dev, 1, n, BF16, init=torch.full((n,), M.GAP))
    nch = table.shape[0]
    nlw = L.load().devit_lamb_workspace(nch, nseg)
    assert nlw == (2 * nch + nseg) * 4
    lws = Out(dev, 1, nlw // 4)
    chunks = table.to(dev)
    nws = L.load().devit_sumsq_workspace()
    ws, gsq = torch.empty(nws, dtype=torch.uint8, device=dev), torch.empty(1, device=dev)
    covered = torch.zeros(n, dtype=torch.bool)
    for o, numel, _ in i["layout"]:
        covered[o:o + numel] = True
    worst = {}
    for step in (1, 2, 3):
        g = i["grads"][step - 1]
        gd = g.to(dev)
        before = {k: t.v[0].cpu().clone() for k, t in st.items()}
        call("devit_sumsq_f32", gd, n, gsq, ws, nws)
        dyn = torch.tensor([hp["lr"], 1 - hp["beta1"] ** step, 1 - hp["beta2"] ** step], dtype=F32, device=dev)
        call("devit_lamb_step", st["p"].t, gd, st["m"].t, st["v"].t, st["ema"].t if c["ema"] else None, p16.t, gsq, dyn, n, chunks, nch, nseg,
             int(c["trust_clip"]), hp["beta1"], hp["beta2"], hp["eps"], hp["wd"], c["max_norm"], hp["ema_decay"], c["grad_scale"], lws.t, nlw)
        ref, bnd = M.lamb_step_bounds(before["p"], g, before["m"], before["v"], before.get("ema"), i["layout"], gsq.cpu(), step, c["max_norm"],
                                      c["grad_scale"], c["trust_clip"])
        got = {k: t.v[0] for k, t in st.items()}
        got["trust"] = lws.v[0, 2 * nch:]
        assert set(ref) == set(got) and lws.intact() and p16.intact()
        for k in ref:
            assert k == "trust" or st[k].intact()
            worst[k] = max(worst.get(k, 0.0), ratio(got[k], ref[k], bnd[k]))
        pc = st["p"].v[0].cpu()
        assert same_bits(p16.v[0].cpu()[covered], pc[covered].to(BF16)), "p_bf16 == bf16(p) on every tensor"
        assert bool((p16.v[0].cpu()[~covered].float() == M.GAP).all()) and bool((pc[~covered] == M.GAP).all()), "the padding belongs to no chunk"
        tr = got["trust"].cpu()
        assert float(tr[6]) == 1.0 and (step > 1 or float(tr[5]) == 1.0)          # everything zero; p = 0 with g != 0 (trust 1 moves it at step 1)
        assert all(float(tr[s]) == 1.0 for s, (_, _, ex) in enumerate(i["layout"]) if ex)
        if c["trust_clip"]:
            assert float(tr.max()) <= 1.0
    assert float(st["p"].v[0].cpu()[slice(i["layout"][6][0], i["layout"][6][0] + 8)].abs().max()) == 0.0          # u = 0: the all-zero tensor stays
    bits = {k: t.v[0].cpu().clone() for k, t in st.items()}
    bits["trust"], bits["p16"] = lws.v[0].cpu().clone(), p16.v[0].cpu().clone()
    return bits, worst


@pytest.mark.parametrize("c", M.lamb_cases(), ids=_lid)
def test_lamb_step(dev, c):
    from devit_amd import optim
    i = M.lamb_inputs(c)
    sizes, offsets = [s for _, s, _ in i["layout"]], [o for o, _, _ in i["layout"]]
    names = [f"t{s}" for s in range(len(sizes))]
    table = optim.lamb_chunk_table(names, sizes, offsets, {nm for nm, (_, _, ex) in zip(names, i["layout"]) if ex})
    optim.validate_chunk_table(table, sizes, offsets, i["n"])
    assert table.shape[0] == 1 + 1 + 1 + 2 + 4 + 3 + 1
    first, worst = _lamb_run(dev, c, i, table)
    _report(f"lamb_step/{_lid(c)}", worst)
    again, _ = _lamb_run(dev, c, i, table)
    for k in first:
        assert torch.equal(first[k].view(torch.int16), again[k].view(torch.int16)), f"{k}: two runs on the same input differ in their bits"


# ============================================================================================ model level
HP = dict(M.OPT_HP, lr=1e-3, wd=0.05, ema_decay=0.999)


@pytest.fixture(scope="module")
def backward(dev):
    """a two-block dedeit at 64 pixels, bs 4, its initial weights and one batch"""
    import devit_amd
    torch.manual_seed(11)
    model = devit_amd.create_model("dedeit", depth=2, num_classes=25, drop_path_rate=0.0, img_size=64)
    g = T.gen("optim_model_level")
    return {k: v.clone() for k, v in model.state_dict().items()}, T.randn(g, 4, 3, 64, 64).to(dev), torch.randint(0, 25, (4,), generator=g).to(dev)


def _ratio_dev(got, ref, bound):
    got = got.to(F64)
    err = (got - ref).abs()
    rt = torch.where(err == 0, torch.zeros_like(err), err / bound)
    rt = torch.where(torch.isfinite(got), rt, torch.full_like(rt, float("inf")))
    return float(rt.max())


@pytest.mark.parametrize("kind", ["nesterov", "adam", "lamb"])
def test_flat_optimizers_behind_a_real_backward(dev, backward, kind):
    """one forward + backward of the model, then one step of the flat optimizer: every parameter, moment and EMA element against the float64 statement
    applied to the fp32 state and the REAL gradients the step started from (the float64 arithmetic runs on the device); the bf16 copy is bf16(p),
    and the k-major fc2 copies the full-row GEMM reads are the transposes of the new bf16 weights"""
    import devit_amd
    from devit_amd import ddp, optim
    state, x, y = backward
    model = devit_amd.create_model("dedeit", depth=2, num_classes=25, drop_path_rate=0.0, img_size=64)
    model.load_state_dict(state)
    model.to(dev).train()
    flat = ddp.FlatParams(model).attach_bf16(model)
    no_decay = optim.no_decay_names(model)
    kw = dict(lr=HP["lr"], weight_decay=HP["wd"], max_norm=1.0, ema_decay=HP["ema_decay"], no_decay=no_decay)
    adam = dict(betas=(HP["beta1"], HP["beta2"]), eps=HP["eps"], **kw)
    opt = {"nesterov": lambda: optim.FlatSGD(flat, momentum=HP["momentum"], nesterov=True, **kw), "adam": lambda: optim.FlatAdam(flat, **adam),
           "lamb": lambda: optim.FlatLamb(flat, **adam)}[kind]()
    opt.zero_grad()
    out = model(x)
    logits = out[0] if isinstance(out, (tuple, list)) else out
    torch.nn.functional.cross_entropy(logits.float(), y).backward()
    keys = opt.state_keys
    s = dict(p=flat.flat.clone(), g=flat.flat_grad.clone(), ema=opt.ema.clone(), **{k: getattr(opt, k).clone() for k in keys})
    assert float(s["g"].abs().max()) > 0 and all(blk.mlp.fc2.__dict__.get("_w16t") is not None for blk in model.blocks)
    opt.step()
    torch.cuda.synchronize()
    gsq = opt.gnorm_sq.cpu()
    ref, bnd = M.sumsq_bounds(s["g"])
    assert chk(ratio(gsq[0], ref, bnd), 1.0, name=f"tail/optim_model/{kind}/gnorm_sq")
    if kind == "nesterov":
        ref, bnd = M.sgd_step_bounds(s["p"], s["g"], s["buf"], s["ema"], opt.no_decay4, gsq, 1, 1.0, 1.0, True, hp=HP)
    elif kind == "adam":
        ref, bnd = M.adam_step_bounds(s["p"], s["g"], s["m"], s["v"], s["ema"], opt.no_decay4, gsq, 1, 1.0, 1.0, hp=HP)
    else:
        layout = [(o, p.numel(), n in no_decay) for n, p, o in zip(flat.names, flat.params, flat.offsets)]
        ref, bnd = M.lamb_step_bounds(s["p"], s["g"], s["m"], s["v"], s["ema"], layout, gsq, 1, 1.0, 1.0, False, hp=HP)
    got = dict(p=flat.flat, ema=opt.ema, **{k: getattr(opt, k) for k in keys})
    if kind == "lamb":
        got["trust"] = opt.trust()
        tr = opt.trust().cpu()
        assert any(float(tr[i]) != 1.0 for i, (_, _, ex) in enumerate(layout) if not ex)
        print("trust ratios of the decayed tensors:", sorted(round(float(tr[i]), 3) for i, (_, _, ex) in enumerate(layout) if not ex))
    worst = {k: _ratio_dev(got[k], ref[k].to(dev), bnd[k].to(dev)) for k in ref}
    _report(f"optim_model/{kind}", worst)
    assert float((flat.flat - s["p"]).abs().max()) > 0
    live = torch.zeros(flat.numel, dtype=torch.bool, device=dev)
    for p, o in zip(flat.params, flat.offsets):
        live[o:o + p.numel()] = True
    assert same_bits(flat.flat16[live], flat.flat[live].to(BF16))
    for blk in model.blocks:
        fc2 = blk.mlp.fc2
        o = flat.offsets[flat.index[id(fc2.weight)]]
        w16 = flat.flat16[o:o + fc2.weight.numel()].view(fc2.weight.shape[0], -1)
        assert fc2._w16[1].data_ptr() == w16.data_ptr() and torch.equal(fc2._w16t[2], w16.t().contiguous()), "the k-major copy follows the step"


# ============================================================================================ the CLIs
BASE = ["--synthetic", "2", "--batch-size", "4", "--model", "dedeit", "--teacher-model", "deit_base_distilled_patch16_224", "--dataset", "cifar100",
        "--num_division", "4", "--warmup-epochs", "0", "--weight-decay", "0.05"]


def _distill(extra):
    import distill_sub
    args = argparse.ArgumentParser(parents=[distill_sub.get_args_parser()]).parse_args(BASE + extra)
    distill_sub.main(args)
    out = os.path.join(args.output_dir, "sub-dataset0")
    lines = [json.loads(l) for l in open(os.path.join(out, "log.txt")).read().splitlines()]
    return args, lines, torch.load(os.path.join(out, "checkpoint_temp.pth"), map_location="cpu", weights_only=False)


@pytest.mark.parametrize("name", ["nesterov", "adam", "lamb"])
def test_distill_sub_with_opt(dev, tmp_path, name):
    a1, lines, ck = _distill(["--epochs", "1", "--opt", name, "--output_dir", str(tmp_path / "a")])
    assert lines[-1]["train_loss"] == lines[-1]["train_loss"] and abs(lines[-1]["train_loss"]) < float("inf")
    assert ck["optimizer"]["opt"] == name and ck["optimizer"]["step"] == 2 and len(ck["model_ema"]) == len(ck["model"])
    state = ("buf",) if name == "nesterov" else ("m", "v")
    assert all(float(ck["optimizer"][k].abs().max()) > 0 for k in state)
    if name != "lamb":
        return
    # --resume of the lamb run: moments, EMA, step count and schedule come back and training continues at the next epoch
    ck_path = os.path.join(a1.output_dir, "sub-dataset0", "checkpoint_temp.pth")
    a2, lines2, ck2 = _distill(["--epochs", "2", "--opt", "lamb", "--output_dir", str(tmp_path / "b"), "--resume", ck_path])
    assert a2.start_epoch == 1 and [l["epoch"] for l in lines2] == [1] and lines2[0]["train_loss"] == lines2[0]["train_loss"]
    assert ck2["optimizer"]["opt"] == "lamb" and ck2["optimizer"]["step"] == 4
    moved = max(float((ck2["model"][k].float() - ck["model"][k].float()).abs().max()) for k in ck["model"])
    assert 0 < moved < 0.1
    import distill_sub
    with pytest.raises(ValueError, match="lamb.*adam"):          # a checkpoint of another kind is refused by name
        distill_sub.main(argparse.ArgumentParser(parents=[distill_sub.get_args_parser()]).parse_args(
            BASE + ["--epochs", "2", "--opt", "adam", "--output_dir", str(tmp_path / "c"), "--resume", ck_path]))


def test_ensemble_with_opt_lamb(dev, tmp_path):
    import ensemble
    parser = argparse.ArgumentParser(parents=[ensemble.get_args_parser()], conflict_handler='resolve')
    args = parser.parse_args(["--synthetic", "2", "--batch-size", "4", "--epochs", "1", "--model", "dedeit", "--opt", "lamb", "--weight-decay", "0.05",
                              "--teacher-model", "deit_base_distilled_patch16_224", "--output_dir", str(tmp_path)])
    args.output_dir = str(tmp_path)
    ensemble.main(args)
    line = json.loads(open(os.path.join(str(tmp_path), "log.txt")).read().splitlines()[-1])
    assert line["train_loss"] == line["train_loss"] and abs(line["train_loss"]) < float("inf") and "test_acc1" in line
    ck = torch.load(os.path.join(str(tmp_path), "checkpoint_temp.pth"), map_location="cpu", weights_only=False)
    opts = [v for v in ck.values() if isinstance(v, dict) and v.get("opt") == "lamb"]
    assert len(opts) == 2, sorted(ck)          # the backbones' optimizer and the fusion head's
