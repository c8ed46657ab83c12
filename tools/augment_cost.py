#!/usr/bin/env python3
"""What the device-resident input stage costs (DESIGN.md sections 15 and 16; results: profiles/augment_cost.json, profiles/randaug_cost.json).

    augment_cost.py kernels [--batch-size 256] [--reps 50]
        cold and warm time of devit_augment_coeffs and of devit_augment_batch (coefficients + resampling) for one batch of 32 x 32 images
        to 224, bicubic, flip and pixel-mode erasing on.  warm: median of back-to-back launches; cold: median of launches that each follow a
        512 MB fill, which leaves nothing of the set, the workspace or the output in the caches.
    augment_cost.py step --source device|synthetic [--steps 30] [--warmup 8]
        bench.py's DEKD step at bs 256 (same models, optimizer, look-ahead teacher, weights put back every step), fed through
        engine._PreparedBatches by a DeviceLoader over a 50 000-image random uint8 set (device) or by resident random batches (synthetic).
        The parent's own yardstick is its bench.py; this leg exists so that the two sources run the very same loop.
    --aa rand-m9-mstd0.5-inc1 (either leg): the image-op layers on (devit_augment_batch_ops; section 16); default: none, the stage of section 15.
One JSON line on stdout."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def kernels(args):
    from devit_amd import _lib as L, data, ops
    dev = torch.device("cuda")
    B, S = args.batch_size, 224
    g = torch.Generator().manual_seed(0)
    ds = data.DeviceImageSet.from_arrays(torch.randint(0, 256, (50000, 32, 32, 3), generator=g, dtype=torch.uint8), torch.zeros(50000, dtype=torch.long), device=dev)
    tf = data.TrainAugment(S, interpolation='bicubic', re_prob=1.0, re_mode='pixel', seed=0, auto_augment=args.aa)
    tab, layers = tf.draw_with_ops(B, 32, 32)
    layers_dev = None if layers is None else data.upload(layers.view(np.uint8).reshape(-1), dev)
    idx = torch.randint(0, 50000, (B,), generator=g, dtype=torch.int32).to(dev)
    tab_dev = data.upload(tab.view(np.uint8).reshape(-1), dev)
    out = torch.empty((B, 3, S, S), device=dev)
    nbytes = L.load().devit_augment_workspace(B, S)
    ws = ops.workspace(dev, nbytes)
    flush = torch.empty(512 << 20, dtype=torch.uint8, device=dev)

    def coeffs():
        ops.call("devit_augment_coeffs", L.ptr(tab_dev), B, S, L.ptr(ws), nbytes, L.stream_ptr())

    def both():
        data.augment_batch(ds.images, idx, tab, S, seed=0, out=out, table_dev=tab_dev, layers=layers, layers_dev=layers_dev)

    def timed(fn, cold):
        ms = []
        for _ in range(args.reps):
            if cold:
                flush.fill_(1)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}
    for fn in (coeffs, both):
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    res = {"what": "kernels", "aa": args.aa or "none", "layers_applied": 0 if layers is None else int(layers["n_ops"].sum()), "batch": B, "source": "32x32 uint8", "S": S, "filter": "bicubic", "erase": "pixel, re_prob 1", "reps": args.reps,
           "erased_share": round(float(sum(int(t["erase"][0][2]) * int(t["erase"][0][3]) for t in tab if t["n_erase"])) / (B * S * S), 4),
           "out_bytes": out.numel() * 4, "workspace_bytes": nbytes,
           "coeffs": {"warm": timed(coeffs, False), "cold": timed(coeffs, True)},
           "coeffs_plus_resample": {"warm": timed(both, False), "cold": timed(both, True)}}
    t0 = time.perf_counter()
    for _ in range(20):
        tf.draw_with_ops(B, 32, 32)
    res["host_draw_ms_per_batch"] = round((time.perf_counter() - t0) / 20 * 1e3, 3)
    print(json.dumps(res))


class _SoftTargets:
    """a loader whose labels become bench.py's fixed soft targets (the step under test is the bench's, which has no Mixup in it)"""

    def __init__(self, loader, soft):
        self.loader, self.soft = loader, soft

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        return ((x, self.soft) for x, _ in self.loader)


def step(args):
    import devit_amd
    import distill_sub
    from devit_amd import data, ddp, engine, losses, optim
    dev = torch.device("cuda")
    B, C, n = args.batch_size, 25, args.warmup + args.steps
    torch.manual_seed(0)
    student = devit_amd.create_model("dedeit", num_classes=C, drop_path_rate=0.1, drop_block_rate=None).to(dev).train()
    torch.manual_seed(1)
    teacher = devit_amd.create_model("deit_base_distilled_patch16_224", num_classes=C).to(dev).eval()
    for p in teacher.parameters():
        p.requires_grad_(False)
    teacher.request_precision("bf16")
    flat = ddp.FlatParams(student)
    ddp.broadcast_parameters(flat)
    flat.attach_bf16(student)
    reducer = ddp.BucketedGradReducer(flat).attach(student)
    opt = optim.FlatAdamW(flat, lr=5e-4 * B / 512.0, weight_decay=0.0, max_norm=1.0, ema_decay=0.99996)
    criterion = losses.DistillLoss(losses.SoftTargetCrossEntropy(), "hard", 0.5, 1.0)
    g = torch.Generator(device=dev).manual_seed(1234)
    y1, y2 = (torch.randint(0, C, (B,), generator=g, device=dev) for _ in range(2))
    oh = lambda y: torch.full((B, C), 0.1 / C, device=dev).scatter_(1, y[:, None], 0.9 + 0.1 / C)
    soft = 0.7 * oh(y1) + 0.3 * oh(y2)
    if args.source == "device":
        gc = torch.Generator().manual_seed(0)
        ds = data.DeviceImageSet.from_arrays(torch.randint(0, 256, (50000, 32, 32, 3), generator=gc, dtype=torch.uint8),
                                             torch.randint(0, C, (50000,), generator=gc), device=dev)
        sampler = torch.randint(0, 50000, (n * B,), generator=gc).tolist()
        loader = data.DeviceLoader(ds, sampler, B, data.TrainAugment(224, re_prob=0.25, re_mode='pixel', seed=0, auto_augment=args.aa), drop_last=True)
    else:
        loader = distill_sub.SyntheticLoader(n, B, C, dev, 1234)
    look = engine.TeacherLookahead(teacher)
    batches = engine._PreparedBatches(_SoftTargets(loader, soft), dev, None, look, row_dtypes=engine.row_dtypes_for(student, teacher))
    feed = iter(batches)
    start_flat, start_flat16 = flat.flat.clone(), flat.flat16.clone()

    def one():
        flat.flat.copy_(start_flat)
        flat.flat16.copy_(start_flat16)
        flat.refresh_kmajor()
        opt.zero_grad()
        x, y, t_out = next(feed)
        out = engine.distill_forward(student, teacher, x, y, gama=(0.2, 0.1, 0.3), criterion=criterion, teacher_outputs=t_out,
                                     after_student=batches.launch_teacher)
        out["loss"].backward()
        reducer.finish()
        opt.step()
        return out["loss"]
    for _ in range(args.warmup):
        one()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        loss = one()
    t_enqueue = time.perf_counter() - t0
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assert bool(torch.isfinite(loss)), "non-finite loss"
    print(json.dumps({"what": "step", "source": args.source, "aa": args.aa or "none", "batch": B, "steps": args.steps, "warmup": args.warmup,
                      "value": round(B * args.steps / dt, 1), "unit": "images/sec", "step_ms": round(dt / args.steps * 1e3, 3),
                      "host_enqueue_ms_per_step": round(t_enqueue / args.steps * 1e3, 3), "loss": float(loss)}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("what", choices=["kernels", "step"])
    ap.add_argument("--source", default="device", choices=["device", "synthetic"])
    ap.add_argument("--batch-size", type=int, default=256)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--aa", default=None, help="a RandAugment config for the device stage, e.g. rand-m9-mstd0.5-inc1 (default: none)")
    a = ap.parse_args()
    (kernels if a.what == "kernels" else step)(a)
