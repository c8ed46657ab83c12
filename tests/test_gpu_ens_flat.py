"""The ensemble stage on the flat fused path, on a real MI355X: the token KL kernel per element against float64 (tests/_ens_model.py), EnsLoss
loss_type='kldiv' against torch's own nn.KLDivLoss in float64 and against the reference's golden step, the optimizer tail of the two clip groups
(all backbones under one norm, the fusion head under its own) against the float64 statements of tests/_optim_model.py on REAL gradients, the closed
loop through engine.train_1epoch_ens_disjoint with ensemble.EnsStepRunner, and the CLI."""
import argparse
import json
import os
import types

import numpy as np
import pytest
import torch

import _ens_model as E
import _optim_model as M
import _tail_model as T
from _tail_model import BF16, F32, F64, U
from conftest import chk
from oracle import devit_oracle as O
from oracle.detgen import det_array
from test_gpu_tail import NAN, Out, call, hold, refused, same_bits

pytestmark = pytest.mark.gpu
TEACHER = "deit_base_distilled_patch16_224"


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from devit_amd import _lib
    _lib.require_device(torch.zeros(1, device="cuda"))
    return torch.device("cuda")


# ============================================================================================ devit_token_kldiv
@pytest.mark.parametrize("n,batch", E.kldiv_cases())
def test_token_kldiv(dev, n, batch):
    i = E.kldiv_inputs(n, batch)
    s, t = i["s"].to(dev), i["t"].to(dev)
    for acc, with_ds in ((0, True), (1, True), (0, False), (1, False)):
        loss, ds = Out(dev, 1, 1, init=i["loss0"] if acc else NAN), Out(dev, 1, n)
        call("devit_token_kldiv", s, t, n, batch, loss.t, ds.t if with_ds else None, acc)
        ref, bnd = E.kldiv_bounds(i["s"], i["t"], batch, i["loss0"] if acc else None)
        assert loss.intact() and ds.intact()
        hold(f"token_kldiv/n{n}_b{batch}_acc{acc}_ds{int(with_ds)}/loss", loss.v[0, 0], ref["loss"], bnd["loss"])
        if with_ds:
            hold(f"token_kldiv/n{n}_b{batch}_acc{acc}/ds", ds.v[0], ref["ds"], bnd["ds"])
        else:
            assert bool(torch.isnan(ds.v).all())


def test_token_kldiv_is_deterministic_and_not_clamped(dev):
    i = E.kldiv_inputs(3073, 7)
    s, t = i["s"].to(dev), i["t"].to(dev)
    a, b = torch.empty(1, device=dev), torch.empty(1, device=dev)
    call("devit_token_kldiv", s, t, 3073, 7, a, None, 0)
    call("devit_token_kldiv", s, t, 3073, 7, b, None, 0)
    assert torch.equal(a, b)
    t2 = t.clone()
    t2[5] = 100.0                                         # exp overflows fp32: torch's loss is inf there, and so is this one
    call("devit_token_kldiv", s, t2, 3073, 7, a, None, 0)
    want = torch.nn.KLDivLoss(reduction="batchmean", log_target=True)(s.view(7, -1), t2.view(7, -1))
    assert not bool(torch.isfinite(a).any()) and not bool(torch.isfinite(want))
    s2 = s.clone()
    s2[9] = NAN
    call("devit_token_kldiv", s2, t, 3073, 7, a, None, 0)
    assert bool(torch.isnan(a).all())


def test_token_kldiv_refusals(dev):
    """the entry point's argument checks: null s / t / loss and n == 0 (DEVIT_ERR_ARG), batch <= 0 and n % batch != 0 (DEVIT_ERR_SHAPE); nothing is
    launched, nothing is written"""
    from devit_amd import _lib as L
    s, t = torch.ones(12, device=dev), torch.ones(12, device=dev)
    loss, ds = Out(dev, 1, 1), Out(dev, 1, 12)
    for a, b, n, batch, lo, code in ((None, t, 12, 3, loss.t, -2), (s, None, 12, 3, loss.t, -2), (s, t, 12, 3, None, -2), (s, t, 0, 3, loss.t, -2),
                                     (s, t, 12, 0, loss.t, -1), (s, t, 12, -2, loss.t, -1), (s, t, 12, 5, loss.t, -1)):
        refused("devit_token_kldiv", a, b, n, batch, lo, ds.t, 0)
        rc = L.load().devit_token_kldiv(L.ptr(a), L.ptr(b), n, batch, L.ptr(lo), L.ptr(ds.t), 0, L.stream_ptr())
        assert rc == code, (n, batch, rc)
    torch.cuda.synchronize()
    assert loss.intact() and ds.intact() and bool(torch.isnan(loss.v).all()) and bool(torch.isnan(ds.v).all()), "a refused call wrote something"


# ============================================================================================ EnsLoss(loss_type='kldiv')
class _StubTeacher(torch.nn.Module):
    def __init__(self, logits, last_tokens):
        super().__init__()
        self.out = dict(output=logits, last_tokens=last_tokens)

    def forward(self, x, distill_token=False):
        return self.out


@pytest.mark.parametrize("model", ["dedeit", "devit"])
def test_ens_loss_kldiv_vs_float64(dev, model):
    """token loss and token gradients of EnsLoss(loss_type='kldiv') against nn.KLDivLoss(reduction="batchmean", log_target=True) in float64, within
    the kernel's bounds (_ens_model.kldiv_bounds; 'dedeit': two pairs accumulated into one scalar, the second launch's accumulate adds 1 rounding,
    counted by passing the first pair's loss as loss0)"""
    from devit_amd import losses
    B, D, C = 4, 768, 10
    g = T.gen("ens_kldiv", model)
    npair = 1 if "vit" in model else 2
    tea = [T.randn(g, B, D) for _ in range(npair)]
    stu = [(tea[k] + T.randn(g, B, D)).to(dev).requires_grad_(True) for k in range(npair)]
    logits = T.randn(g, B, C).to(dev).requires_grad_(True)
    tea_dev = [x.to(dev) for x in tea]
    teacher = _StubTeacher(T.randn(g, B, C).to(dev), tea_dev[0] if npair == 1 else tuple(tea_dev))
    crit = losses.EnsLoss(torch.nn.CrossEntropyLoss(), teacher, model, "hard", 0.5, 1.0, loss_type="kldiv")
    y = torch.randint(0, C, (B,), generator=g).to(dev)
    token_loss, cls_loss = crit(None, (stu[0] if npair == 1 else tuple(stu), logits), y)
    (token_loss + cls_loss).backward()
    kl = torch.nn.KLDivLoss(reduction="batchmean", log_target=True)
    ref_loss, bnd_loss = 0.0, 0.0
    for k in range(npair):
        s64 = stu[k].detach().cpu().to(F64).requires_grad_(True)
        l64 = kl(s64, tea[k].to(F64))
        l64.backward()
        ref, bnd = E.kldiv_bounds(stu[k].detach().cpu().reshape(-1), tea[k].reshape(-1), B, None if k == 0 else torch.tensor([ref_loss], dtype=F64))
        assert abs(float(l64.detach()) + ref_loss - float(ref["loss"])) <= 1e-9 * float(bnd["loss"]) / U
        ref_loss, bnd_loss = float(ref["loss"]), bnd_loss + float(bnd["loss"])
        hold(f"ens_loss_kldiv/{model}/dtoken{k}", stu[k].grad.reshape(-1), s64.grad.reshape(-1), bnd["ds"] + U * ref["ds"].abs())   # (+1: times the upstream 1.0)
    hold(f"ens_loss_kldiv/{model}/token_loss", token_loss.detach(), ref_loss, bnd_loss)
    assert logits.grad is not None and bool(torch.isfinite(cls_loss))


def rel(a, b):
    a = a.detach().float().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def test_ensemble_kldiv_vs_golden(golden, dev):
    """The whole step of tests/test_gpu_model.py::test_ensemble_vs_golden (4 x dedeit + EnsMLP + DeiT-B teacher, bs 4, hard distillation) with
    the reference's own EnsLoss(loss_type='kldiv') (tests/golden/make_golden_kldiv.py), at that test's bars: 2e-2 on the losses, 2.5e-2 on the
    gradient slices."""
    import devit_amd
    from devit_amd import engine, losses
    from devit_amd.ensemble_models import EnsMLP, MultiViT, load_sub_checkpoints
    g = golden("ensemble_kldiv")
    GS, GT = O.GEOMETRY["dedeit"], O.GEOMETRY[TEACHER]
    multi = MultiViT("dedeit", drop=0, drop_path=0.0, num_classes_list=[25] * 4, num_div=4)
    load_sub_checkpoints(multi, [O.make_state(GS, 25, f"E{i}") for i in range(4)])
    ens = EnsMLP("dedeit", 100, 384, [25] * 4, 768)
    ens.load_state_dict(O.make_ens_state())
    teacher = devit_amd.create_model(TEACHER, num_classes=100)
    teacher.load_state_dict(O.make_state(GT, 100, "T100"))
    multi.to(dev).train(); ens.to(dev).train(); teacher.to(dev).eval()
    img = torch.from_numpy(det_array("img4", (4, 3, 224, 224))).to(dev)
    crit = losses.EnsLoss(losses.SoftTargetCrossEntropy(), teacher, "dedeit", "hard", 0.5, 1.0, loss_type="kldiv")
    out = engine.ens_forward(multi, ens, crit, img, torch.from_numpy(g["soft_targets"]).to(dev))
    out["loss"].backward()
    e_tok = abs(float(out["token_loss"]) - float(g["token_loss"])) / abs(float(g["token_loss"]))
    e_cls = abs(float(out["cls_loss"]) - float(g["cls_loss"])) / abs(float(g["cls_loss"]))
    slices = dict(g_cls_mlp_w_rows=ens.cls_mlp.weight.grad[::48], g_dist_cls_w=ens.dist_classifier.weight.grad[::10],
                  g_b2_fc1_rows=multi.backbones[2].blocks[3].mlp.fc1.weight.grad[::96], g_b0_pos=multi.backbones[0].pos_embed.grad[0, ::16])
    errs = {k: rel(v, g[k]) for k, v in slices.items()}
    print(f"ensemble_kldiv: token_loss {float(out['token_loss']):.4f} vs {float(g['token_loss']):.4f} ({e_tok:.3e}), cls_loss {e_cls:.3e}, slices {errs}")
    ok = chk(e_tok, 2e-2, name="ens_kldiv_golden/token_loss") & chk(e_cls, 2e-2, name="ens_kldiv_golden/cls_loss")
    for k, v in errs.items():
        ok &= chk(v, 2.5e-2, name=f"ens_kldiv_golden/{k}")
    assert ok, (e_tok, e_cls, errs)


# ============================================================================================ the optimizer tail, two clip groups
IMG, B, NCLS = 64, 4, 10
HP = dict(beta1=0.9, beta2=0.999, eps=1e-8, wd=0.05, ema_decay=0.99996, lr=1e-4)


@pytest.fixture(scope="module")
def setup(dev):
    """initial weights of MultiViT(2 x dedeit) + EnsMLP at 64 pixels (kept on the CPU: every run starts from them), the frozen DeiT-B teacher, and
    three batches"""
    import devit_amd
    from devit_amd.ensemble_models import EnsMLP, MultiViT
    torch.manual_seed(7)
    multi = MultiViT("dedeit", num_div=2, drop_path=0, num_classes_list=[5, 5], img_size=IMG)
    ens = EnsMLP("dedeit", NCLS, 384, [5, 5], 768)
    teacher = devit_amd.create_model(TEACHER, num_classes=NCLS, img_size=IMG).to(dev).eval()
    for p in teacher.parameters():
        p.requires_grad_(False)
    g = T.gen("ens_flat_batches")
    batches = [(T.randn(g, B, 3, IMG, IMG).to(dev), torch.randint(0, NCLS, (B,), generator=g).to(dev)) for _ in range(3)]
    return dict(multi={k: v.clone() for k, v in multi.state_dict().items()}, ens={k: v.clone() for k, v in ens.state_dict().items()},
                teacher=teacher, batches=batches)


def _fresh(setup, dev):
    from devit_amd import losses
    from devit_amd.ensemble_models import EnsMLP, MultiViT
    multi = MultiViT("dedeit", num_div=2, drop_path=0, num_classes_list=[5, 5], img_size=IMG)
    ens = EnsMLP("dedeit", NCLS, 384, [5, 5], 768)
    multi.load_state_dict(setup["multi"]); ens.load_state_dict(setup["ens"])
    multi.to(dev).train(); ens.to(dev).train()
    crit = losses.EnsLoss(torch.nn.CrossEntropyLoss(), setup["teacher"], "dedeit", "hard", 0.5, 1.0)
    return multi, ens, crit


def _flat_tail(multi, ens, max_norm=1.0):
    import ensemble
    from devit_amd import ddp, optim
    flat, ens_flat = ddp.FlatParams(multi).attach_bf16(multi), ddp.FlatParams(ens)
    runner = ensemble.EnsStepRunner(ddp.BucketedGradReducer(flat).attach(multi), ddp.BucketedGradReducer(ens_flat))
    kw = dict(lr=HP["lr"], betas=(HP["beta1"], HP["beta2"]), eps=HP["eps"], weight_decay=HP["wd"], max_norm=max_norm, ema_decay=HP["ema_decay"])
    return flat, ens_flat, runner, optim.FlatAdamW(flat, no_decay=optim.no_decay_names(multi), **kw), \
        optim.FlatAdamW(ens_flat, no_decay=optim.no_decay_names(ens), **kw)


def _ratio_dev(got, ref, bound):
    """_tail_model.ratio on the device (44 M elements): 0 / 0 -> 0, x / 0 -> inf, a non-finite output -> inf"""
    got = got.to(F64)
    err = (got - ref).abs()
    rt = torch.where(err == 0, torch.zeros_like(err), err / bound)
    rt = torch.where(torch.isfinite(got), rt, torch.full_like(rt, float("inf")))
    return float(rt.max())


def test_fused_tail_two_clip_groups(setup, dev):
    """One ens_forward + backward, then one fused step per group (max_norm 1.0, weight decay 0.05, EMA 0.99996), each held to the float64 statement
    of the optimizer kernels applied to the fp32 state and the REAL gradients the step started from: the group's norm (sumsq_bounds), p / m / v /
    ema (adamw_step_bounds with the group's own gnorm_sq) and the bf16 copy (bit-exact bf16(p)).  The float64 arithmetic runs on the device."""
    from devit_amd import engine
    multi, ens, crit = _fresh(setup, dev)
    flat, ens_flat, runner, opt, ens_opt = _flat_tail(multi, ens)
    x, y = setup["batches"][0]
    out = engine.ens_forward(multi, ens, crit, x, y, "hard")
    snaps = []
    for f, o in ((flat, opt), (ens_flat, ens_opt)):
        o.zero_grad()
    out["loss"].backward()
    for f, o in ((flat, opt), (ens_flat, ens_opt)):
        snaps.append(dict(p=f.flat.clone(), g=f.flat_grad.clone(), m=o.m.clone(), v=o.v.clone(), ema=o.ema.clone()))
    runner.reducer.finish(); runner.ens_reducer.finish()
    for o in (opt, ens_opt):
        o.step()
    torch.cuda.synchronize()
    assert opt.gnorm_sq.data_ptr() != ens_opt.gnorm_sq.data_ptr()
    # the backbones' norm is ONE norm over both backbones: the sum of the two per-backbone sums, not either of them
    per_bb = [sum(float((p.grad.double() ** 2).sum()) for p in m.parameters()) for m in multi.backbones]
    assert min(per_bb) > 0 and abs(float(opt.gnorm_sq) - sum(per_bb)) < 1e-4 * sum(per_bb)
    for name, f, o, s in (("backbones", flat, opt, snaps[0]), ("ens_mlp", ens_flat, ens_opt, snaps[1])):
        ref, bnd = M.sumsq_bounds(s["g"])
        hold(f"ens_tail/{name}/gnorm_sq", o.gnorm_sq[0], ref, bnd)
        assert float(o.gnorm_sq) > 0
        ref, bnd = M.adamw_step_bounds(s["p"], s["g"], s["m"], s["v"], s["ema"], o.no_decay4, o.gnorm_sq.cpu(), 1, 1.0, 1.0, hp=HP)
        got = dict(p=f.flat, m=o.m, v=o.v, ema=o.ema)
        for k in ("p", "m", "v", "ema"):
            r = _ratio_dev(got[k], ref[k], bnd[k])
            print(f"tail/ens_tail/{name}/{k} {r:.3f}")
            assert chk(r, 1.0, name=f"tail/ens_tail/{name}/{k}"), (name, k, r)
        assert float((f.flat - s["p"]).abs().max()) > 0
    assert same_bits(flat.flat16, flat.flat.to(BF16)) and ens_flat.flat16 is None
    clipped = float(opt.gnorm_sq) > 1.0 or float(ens_opt.gnorm_sq) > 1.0
    print(f"gradient norms: backbones {float(opt.gnorm_sq) ** 0.5:.4f}, fusion head {float(ens_opt.gnorm_sq) ** 0.5:.4f} (clip at 1.0 bites: {clipped})")


# ============================================================================================ closed loop
def _one_step_loaders(setup):
    return [[b] for b in setup["batches"]]


def _torch_tail_losses(setup, dev):
    import ensemble
    from devit_amd import engine
    multi, ens, crit = _fresh(setup, dev)
    kw = dict(lr=HP["lr"], eps=HP["eps"], betas=(HP["beta1"], HP["beta2"]))
    opt = torch.optim.AdamW(ensemble.param_groups(multi, HP["wd"]), **kw)
    ens_opt = torch.optim.AdamW(ensemble.param_groups(ens, HP["wd"]), **kw)
    args = types.SimpleNamespace(distillation_type="hard")
    return [engine.train_1epoch_ens_disjoint(multi, ens, crit, loader, opt, ens_opt, dev, 0, None, args, None, max_norm=1.0)["loss"]
            for loader in _one_step_loaders(setup)]


# of |loss|, per step.  Measured on MI355X: the fused tail's loss curve deviates from the torch tail's by 1.23e-4 (step 1 is bit-identical, the
# weights differ from step 2 on by the rounding of two different but equivalent update formulas); the torch tail's own run-to-run spread over
# two runs is 0 at this size.  The bar is twice the larger; the ceiling it must stay under is the 2e-2 of "one training, two ways".
CLOSED_LOOP_BAR = 2.5e-4


def test_closed_loop_fused_vs_torch_tail(setup, dev):
    """Three steps through engine.train_1epoch_ens_disjoint with ensemble.EnsStepRunner (lr 1e-4, clip 1.0, weight decay 0.05, EMA), the
    invariants of the flat path after every step, and the loss curve against torch's tail (two AdamW + clip_grad_norm_) from the same weights."""
    from devit_amd import de_vit, engine
    multi, ens, crit = _fresh(setup, dev)
    flat, ens_flat, runner, opt, ens_opt = _flat_tail(multi, ens)
    linears = [m for bb in multi.backbones for m in bb.modules() if isinstance(m, (torch.nn.Linear, torch.nn.Conv2d))]
    assert len(linears) == 2 * (12 * 4 + 1)
    fc2s = [blk.mlp.fc2 for bb in multi.backbones for blk in bb.blocks]
    for m in fc2s:                    # the k-major copies the full-row GEMM reads at training sizes (these 72-row batches run the tile kernels)
        de_vit._w16t(m, m._w16[1])
    args = types.SimpleNamespace(distillation_type="hard")
    lo16, hi16 = flat.flat16.data_ptr(), flat.flat16.data_ptr() + 2 * flat.numel
    d = HP["ema_decay"]
    losses, ptrs = [], []
    for step, loader in enumerate(_one_step_loaders(setup), 1):
        ema0, ens_ema0 = opt.ema[:65536].clone(), ens_opt.ema[:65536].clone()
        stats = engine.train_1epoch_ens_disjoint(multi, ens, crit, loader, opt, ens_opt, dev, 0, runner, args, None, max_norm=1.0)
        losses.append(stats["loss"])
        assert same_bits(flat.flat16, flat.flat.to(BF16)), f"step {step}: flat16 != bf16(masters)"
        ptrs.append([m._w16[1].data_ptr() for m in linears])
        for m in linears:
            w16 = m._w16[1]
            o = flat.offsets[flat.index[id(m.weight)]]
            assert w16.data_ptr() == lo16 + 2 * o and w16.data_ptr() + 2 * w16.numel() <= hi16, "a GEMM weight copy outside flat16"
        for m in fc2s:
            c = m.__dict__["_w16t"]
            assert c[0] == m._w16[1].data_ptr() and torch.equal(c[2], m._w16[1].t()), f"step {step}: a stale k-major copy"
        for o_, f_, e0 in ((opt, flat, ema0), (ens_opt, ens_flat, ens_ema0)):
            e0, p1 = e0.to(F64), f_.flat[:65536].to(F64)
            ref = e0 * T._f(d) + T._f(1.0 - T._f(d)) * p1
            bnd = U * ((e0 * d).abs() + ((1 - d) * p1).abs()) + U * ref.abs()
            assert _ratio_dev(o_.ema[:65536], ref, bnd) <= 1.0 and float((o_.ema[:65536] - e0.float()).abs().max()) > 0, f"step {step}: EMA recurrence"
        if step == 1:
            dead = [n for mod in (multi, ens) for n, p in mod.named_parameters() if p.requires_grad and not float(p.grad.abs().max()) > 0]
            assert not dead, f"parameters without a gradient (a flat buffer would decay them, torch AdamW would skip them): {dead}"
    assert ptrs[0] == ptrs[2]
    ref_a, ref_b = _torch_tail_losses(setup, dev), _torch_tail_losses(setup, dev)
    dev_fused = max(abs(a - b) / abs(b) for a, b in zip(losses, ref_a))
    spread = max(abs(a - b) / abs(b) for a, b in zip(ref_a, ref_b))
    print(f"closed loop: fused {losses} torch tail {ref_a} / {ref_b}: deviation {dev_fused:.3e}, torch tail's run-to-run spread {spread:.3e}")
    chk(spread, CLOSED_LOOP_BAR, name="ens_closed_loop/torch_tail_run_to_run")
    assert losses[0] != losses[2] and all(np.isfinite(losses))
    assert CLOSED_LOOP_BAR <= 2e-2 and spread <= CLOSED_LOOP_BAR
    assert chk(dev_fused, CLOSED_LOOP_BAR, name="ens_closed_loop/fused_vs_torch_tail"), (dev_fused, spread)


# ============================================================================================ CLI
def _cli(tmp_path, name, extra):
    import ensemble
    out = tmp_path / name
    os.makedirs(out)
    parser = argparse.ArgumentParser(parents=[ensemble.get_args_parser()], conflict_handler="resolve")
    a = parser.parse_args(["--synthetic", "2", "--batch-size", "4", "--epochs", "1", "--input-size", "64", "--model", "dedeit",
                           "--teacher-model", TEACHER, "--output_dir", str(out)] + extra)
    a.output_dir = str(out)
    ensemble.main(a)
    line = json.loads(open(out / "log.txt").read().splitlines()[-1])
    return line, torch.load(out / "checkpoint_temp.pth", map_location="cpu", weights_only=False)


OLD_KEYS = {"model", "ens_model", "optimizer", "ens_optimizer", "lr_scheduler", "ens_lr_scheduler", "epoch", "scaler", "args"}


def test_cli_kldiv_and_ema(dev, tmp_path):
    line, ck = _cli(tmp_path, "kldiv", ["--loss", "kldiv"])
    assert np.isfinite(line["train_token_loss"]) and np.isfinite(line["train_loss"]) and "test_acc1" in line
    assert set(ck) == OLD_KEYS | {"model_ema", "ens_model_ema"}
    assert set(ck["model_ema"]) == set(ck["model"]) and set(ck["ens_model_ema"]) == set(ck["ens_model"])
    k = "backbones.3.blocks.0.attn.qkv.weight"
    gap = float((ck["model_ema"][k] - ck["model"][k]).abs().max())
    assert 0 < gap < 1e-2                                # the EMA trails the weights
    line, ck = _cli(tmp_path, "noema", ["--no-model-ema"])
    assert ck.get("model_ema") is None and ck.get("ens_model_ema") is None and np.isfinite(line["train_loss"])


def test_cli_torch_optim_keeps_the_old_tail(dev, tmp_path):
    line, ck = _cli(tmp_path, "torch", ["--torch-optim"])
    assert set(ck) == OLD_KEYS and "state" in ck["optimizer"] and np.isfinite(line["train_loss"])


def test_cli_trains_through_compacted_backbones(dev, tmp_path, capsys):
    """--gates F --physical-shrink without --eval: 4 of 6 heads and 1024 of 1536 neurons per block (as test_ensemble_cli_checkpoints_gates_shrink);
    train_loss within 2e-2 of the masked run's (one training, two ways: the bar of test_gpu_cli.py)."""
    from devit_amd import shrink
    from devit_amd.ensemble_models import MultiViT
    multi = MultiViT(model="dedeit", num_div=4, num_classes_list=[25] * 4, img_size=64)
    g = torch.Generator().manual_seed(3)
    pol = []
    for _ in range(4 * 12):
        h, n = torch.zeros(6), torch.zeros(1536)
        h[torch.randperm(6, generator=g)[:4]] = 1
        n[torch.randperm(1536, generator=g)[:1024]] = 1
        pol.append((h, n))
    shrink.load_policy(multi, pol)
    shrink.save_gates(multi, tmp_path / "gates.pt")
    common = ["--gates", str(tmp_path / "gates.pt"), "--drop-path", "0", "--mixup", "0", "--cutmix", "0", "--seed", "3"]
    capsys.readouterr()
    masked, _ = _cli(tmp_path, "masked", common + ["--no-physical-shrink"])
    assert "compacted" not in capsys.readouterr().out
    compact, _ = _cli(tmp_path, "compact", common + ["--physical-shrink"])
    assert "shrink: compacted 48 blocks for training" in capsys.readouterr().out
    e = abs(compact["train_loss"] - masked["train_loss"]) / abs(masked["train_loss"])
    print(f"train_loss masked {masked['train_loss']:.6f} compacted {compact['train_loss']:.6f} ({e:.3e})")
    assert chk(e, 2e-2, name="ens_cli/compact_vs_masked_train_loss")
