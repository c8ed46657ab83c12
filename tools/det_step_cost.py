#!/usr/bin/env python3
"""What deterministic mode costs in the step: the bs-256 DEKD step -- forward + backward + the fused AdamW tail with EMA -- with the mode off and on,
five rounds that alternate the two on one box, each sample the mean of ITERS iterations between two events; medians, ranges, the ratio against the
mode off and the peak allocated memory of each mode go to OUT.json (profiles/det_step_cost.json).  usage: det_step_cost.py [OUT.json]"""
import json
import os
import statistics as st
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import devit_amd  # noqa: E402
from devit_amd import ddp, engine, ops, optim  # noqa: E402

dev = torch.device("cuda")
B, C, ROUNDS, ITERS = 256, 25, 5, 4
torch.manual_seed(0)
student = devit_amd.create_model("dedeit", num_classes=C, drop_path_rate=0.1).to(dev).train()
teacher = devit_amd.create_model("deit_base_distilled_patch16_224", num_classes=C).to(dev).eval()
for p in teacher.parameters():
    p.requires_grad_(False)
flat = ddp.FlatParams(student).attach_bf16(student)
reducer = ddp.BucketedGradReducer(flat).attach(student)
opt = optim.FlatAdamW(flat, lr=1e-4, weight_decay=0.05, max_norm=1.0, ema_decay=0.99996, no_decay=optim.no_decay_names(student))
img = torch.randn(B, 3, 224, 224, device=dev)
soft = torch.nn.functional.one_hot(torch.randint(0, C, (B,), device=dev), C).float() * 0.9 + 0.1 / C


def step():
    opt.zero_grad()
    engine.distill_forward(student, teacher, img, soft)["loss"].backward()
    reducer.finish()
    opt.step()


def sample(on):
    with ops.deterministic(on):
        step()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(ITERS):
            step()
        e1.record()
        torch.cuda.synchronize()
    return e0.elapsed_time(e1) / ITERS, torch.cuda.max_memory_allocated() / 2 ** 30


CONFIGS = {"default": False, "deterministic": True}
samples, peak = {k: [] for k in CONFIGS}, {}
for k, on in CONFIGS.items():          # first calls (allocator, module load, the workspace) are not samples; the mode off comes first: its peak is the
    peak["before_the_workspace" if not on else "first_deterministic"] = round(sample(on)[1], 3)      # step's without the workspace
for _ in range(ROUNDS):
    for k, on in CONFIGS.items():
        ms, gb = sample(on)
        samples[k].append(round(ms, 3))
        peak[k] = round(max(peak.get(k, 0.0), gb), 3)
res = {"dekd_step_ms": {k: dict(samples=v, median=round(st.median(v), 3), min=min(v), max=max(v)) for k, v in samples.items()}}
res["ratio_vs_default"] = round(res["dekd_step_ms"]["deterministic"]["median"] / res["dekd_step_ms"]["default"]["median"], 4)
res["peak_allocated_gib"] = peak          # (the mode's registered workspace, devit_det_workspace_bytes(), stays allocated once it exists: both figures hold it)
res["workspace_mib"] = ops.L.load().devit_det_workspace_bytes() >> 20
res["shape"] = dict(B=B, N=198, student="dedeit", teacher="deit_base_distilled_patch16_224", rounds=ROUNDS, iters_per_sample=ITERS,
                    optimizer="FlatAdamW + EMA, max_norm 1.0", wgrad_group=os.environ.get("DEVIT_WGRAD_GROUP", "auto"))
txt = json.dumps(res, indent=1)
print(txt)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write(txt + "\n")
