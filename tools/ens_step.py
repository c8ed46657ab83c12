#!/usr/bin/env python3
"""ms / step of the ensemble TRAINING step (BASELINE config 5: MultiViT of 4 x dedeit + EnsMLP under a DeiT-B teacher, bs 256, hard
distillation, token MSE, synthetic data) with the two optimizer tails ensemble.py can run: the flat fused tail (default) and torch's
(--torch-optim: two torch.optim.AdamW over the separate tensors).  No figure is promised: this reports what they measure.

    python tools/ens_step.py --rounds 5 --out profiles/ens_flat_step.json      # alternating rounds, each measurement a child process under `timeout`
    python tools/ens_step.py --tail fused --steps 20 --warmup 5                # one measurement, one JSON line

Launch counts: for the fused tail the C-ABI calls between the end of backward and the end of the step (devit_sumsq_f32, devit_adamw_step, the
k-major refresh); for torch's tail the tensors its optimizers update one by one, and the bf16 re-casts / k-major re-transposes the NEXT forward
has to redo because every in-place update bumped a weight's version (counted at the Python entry points ops.cast_bf16 / ops.transpose16)."""
import argparse
import json
import os
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TEACHER = "deit_base_distilled_patch16_224"


def measure(tail, B, steps, warmup, dev):
    import devit_amd
    import ensemble
    from devit_amd import ddp, engine, losses, ops, optim
    from devit_amd.ensemble_models import EnsMLP, MultiViT
    C, subs = 100, [25] * 4
    torch.manual_seed(0)
    multi = MultiViT("dedeit", num_div=4, num_classes_list=subs).to(dev).train()
    ens = EnsMLP("dedeit", C, 384, subs, 768).to(dev).train()
    teacher = devit_amd.create_model(TEACHER, num_classes=C).to(dev).eval()
    for p in teacher.parameters():
        p.requires_grad_(False)
    crit = losses.EnsLoss(torch.nn.CrossEntropyLoss(), teacher, "dedeit", "hard", 0.5, 1.0, "mse")
    lr, wd, betas = 1e-5 * B / 512.0, 0.05, (0.9, 0.999)
    counts = {}
    if tail == "fused":
        flat, ens_flat = ddp.FlatParams(multi).attach_bf16(multi), ddp.FlatParams(ens)
        runner = ensemble.EnsStepRunner(ddp.BucketedGradReducer(flat).attach(multi), ddp.BucketedGradReducer(ens_flat))
        opt = optim.FlatAdamW(flat, lr=lr, betas=betas, weight_decay=wd, max_norm=1.0, ema_decay=0.99996, no_decay=optim.no_decay_names(multi))
        ens_opt = optim.FlatAdamW(ens_flat, lr=lr, betas=betas, weight_decay=wd, max_norm=1.0, ema_decay=0.99996, no_decay=optim.no_decay_names(ens))
    else:
        runner = None
        opt = torch.optim.AdamW(ensemble.param_groups(multi, wd), lr=lr, betas=betas)
        ens_opt = torch.optim.AdamW(ensemble.param_groups(ens, wd), lr=lr, betas=betas)
    g = torch.Generator(device=dev).manual_seed(1234)
    img = torch.randn((B, 3, 224, 224), generator=g, device=dev)
    y = torch.randint(0, C, (B,), generator=g, device=dev)

    def step():
        opt.zero_grad(set_to_none=True)
        ens_opt.zero_grad(set_to_none=True)
        out = engine.ens_forward(multi, ens, crit, img, y, "hard")
        if runner is not None:
            runner(out["loss"], opt, ens_opt, clip_grad=1.0)
        else:
            out["loss"].backward()
            torch.nn.utils.clip_grad_norm_(multi.parameters(), 1.0)
            torch.nn.utils.clip_grad_norm_(ens.parameters(), 1.0)
            opt.step()
            ens_opt.step()
        return out["loss"]

    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        loss = step()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    # one more step with the entry points counted
    seen = []
    real_call, real_ops_call, real_cast, real_tr = optim.call, ops.call, ops.cast_bf16, ops.transpose16
    if tail == "fused":
        real_bwd = torch.Tensor.backward
        after = [False]

        def backward(self, *a, **k):
            real_bwd(self, *a, **k)
            after[0] = True
        rec = lambda real: (lambda name, *a: (seen.append(name) if after[0] else None, real(name, *a))[1])
        torch.Tensor.backward, optim.call, ops.call = backward, rec(real_call), rec(real_ops_call)
        try:
            step()
        finally:
            torch.Tensor.backward, optim.call, ops.call = real_bwd, real_call, real_ops_call
        counts = {n: seen.count(n) for n in sorted(set(seen))}
    else:
        ops.cast_bf16 = lambda *a, **k: (seen.append("cast_bf16"), real_cast(*a, **k))[1]
        ops.transpose16 = lambda *a, **k: (seen.append("transpose16"), real_tr(*a, **k))[1]
        try:
            step()
        finally:
            ops.cast_bf16, ops.transpose16 = real_cast, real_tr
        counts = {"tensors_updated_one_by_one": sum(len(g_["params"]) for o in (opt, ens_opt) for g_ in o.param_groups),
                  "clip_grad_norm_calls": 2, "cast_bf16_in_next_forward": seen.count("cast_bf16"),
                  "transpose16_in_next_forward": seen.count("transpose16")}
    torch.cuda.synchronize()
    loss = float(loss.detach())
    assert loss == loss, "non-finite loss"
    return {"tail": tail, "batch_size": B, "steps": steps, "ms_per_step": round(dt / steps * 1e3, 3), "img_per_s": round(B * steps / dt, 1),
            "loss": loss, "tail_launch_counts": counts}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tail", choices=["fused", "torch"], default=None, help="one measurement in this process")
    ap.add_argument("--rounds", type=int, default=5, help="alternating torch / fused rounds, one child process each")
    ap.add_argument("--batch-size", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per child")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.tail is not None:
        assert torch.cuda.is_available(), "needs an MI355X"
        print(json.dumps(measure(a.tail, a.batch_size, a.steps, a.warmup, torch.device("cuda", 0))))
        return
    rows = []
    for r in range(a.rounds):
        for tail in ("torch", "fused"):
            cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--tail", tail, "--batch-size", str(a.batch_size),
                   "--steps", str(a.steps), "--warmup", str(a.warmup)]
            p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
            if p.returncode != 0:            # a fault, an abort or the time limit: nothing more is started on the GPU
                raise SystemExit(f"round {r} {tail}: exit status {p.returncode}; stopping")
            rows.append(dict(json.loads(p.stdout.strip().splitlines()[-1]), round=r))
            print(rows[-1], flush=True)
    ms = {t: [x["ms_per_step"] for x in rows if x["tail"] == t] for t in ("torch", "fused")}
    doc = {"what": "ensemble training step, 4 x dedeit + EnsMLP under DeiT-B, bs %d, hard distillation, token MSE, clip 1.0, weight decay 0.05; host clock "
                   "around %d steps ending in a synchronise, %d alternating rounds of one child process each" % (a.batch_size, a.steps, a.rounds),
           "ms_per_step_range": {t: [min(v), max(v)] for t, v in ms.items()},
           "tail_launch_counts": {t: next(x["tail_launch_counts"] for x in rows if x["tail"] == t) for t in ("torch", "fused")}, "rows": rows}
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
