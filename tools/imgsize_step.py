#!/usr/bin/env python3
"""img/s of one DEKD step (`dedeit` under DeiT-B, bs 256, C = 25) at several image sizes, next to 224: bench.py's step -- the same models,
look-ahead teacher, one im2row pass per batch, fused optimizer, the weights put back before every step -- with `img_size=S` models and
S x S batches.  Writes one JSON document (profiles/imgsize_step.json is a committed copy).  Needs an MI355X; no figure is promised for the
sizes other than 224, this reports what they measure.

    python tools/imgsize_step.py --sizes 112 160 224 --steps 20 --warmup 5 --out imgsize_step.json
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def measure(S, B, C, steps, warmup, dev):
    import devit_amd
    from devit_amd import ddp, engine, flops, losses, ops, optim
    torch.manual_seed(0)
    student = devit_amd.create_model("dedeit", num_classes=C, drop_path_rate=0.1, drop_block_rate=None, img_size=S).to(dev).train()
    torch.manual_seed(1)
    teacher = devit_amd.create_model("deit_base_distilled_patch16_224", num_classes=C, img_size=S).to(dev).eval()
    for p in teacher.parameters():
        p.requires_grad_(False)
    flat = ddp.FlatParams(student)
    flat.attach_bf16(student)
    reducer = ddp.BucketedGradReducer(flat).attach(student)
    opt = optim.FlatAdamW(flat, lr=5e-4 * B / 512.0, weight_decay=0.0, max_norm=1.0, ema_decay=0.99996)
    criterion = losses.DistillLoss(losses.SoftTargetCrossEntropy(), "hard", 0.5, 1.0)
    g = torch.Generator(device=dev).manual_seed(1234)
    img = torch.randn((B, 3, S, S), generator=g, device=dev)
    y1, y2 = (torch.randint(0, C, (B,), generator=g, device=dev) for _ in range(2))
    oh = lambda y: torch.full((B, C), 0.1 / C, device=dev).scatter_(1, y[:, None], 0.9 + 0.1 / C)
    soft = 0.7 * oh(y1) + 0.3 * oh(y2)
    look = engine.TeacherLookahead(teacher)
    row_dtypes = engine.row_dtypes_for(student, teacher)
    prepare = lambda: ops.patch_rows(img, dtypes=row_dtypes)
    state = {"cur": prepare()}
    look.submit(state["cur"])
    start_flat, start_flat16 = flat.flat.clone(), flat.flat16.clone()

    def step():
        flat.flat.copy_(start_flat)
        flat.flat16.copy_(start_flat16)
        flat.refresh_kmajor()
        opt.zero_grad()
        x, t_out = state["cur"], look.take(state["cur"])
        state["cur"] = prepare()
        look.submit(state["cur"], defer=True)
        out = engine.distill_forward(student, teacher, x, soft, gama=(0.2, 0.1, 0.3), criterion=criterion, teacher_outputs=t_out,
                                     after_student=look.launch)
        out["loss"].backward()
        reducer.finish()
        opt.step()
        return out["loss"]

    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        loss = step()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    look.take(state["cur"])
    loss = float(loss.detach())
    assert loss == loss, "non-finite loss"
    tokens = flops.seq_length_for(S, 2)
    return {"img_size": S, "tokens": tokens, "batch_size": B, "steps": steps, "img_per_s": round(B * steps / dt, 1),
            "ms_per_step": round(dt / steps * 1e3, 3), "gflop_per_img_step": round(flops.step_gflops_per_image(C, tokens, S), 3), "loss": loss}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[112, 160, 224])
    ap.add_argument("--batch-size", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda", 0)
    rows = [measure(S, a.batch_size, 25, a.steps, a.warmup, dev) for S in a.sizes]
    doc = {"what": "one DEKD step, dedeit under DeiT-B, C = 25, look-ahead teacher; host clock around steps ending in a synchronise", "rows": rows}
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
