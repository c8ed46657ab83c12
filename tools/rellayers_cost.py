#!/usr/bin/env python3
"""What --relation-layers costs in the step: the DEKD step's forward + backward (student + teacher + losses; the optimizer does not depend on the
selection) at bs 256, 224 pixels, with the selections mid, last and all, ROUNDS rounds that alternate the three on one box, each sample the mean of
ITERS iterations between two events.  Beside the measurement, the estimates it is held against: `all` is eleven more relation forward + backward
pairs, `last` gives up the lean tail's saving (flops.lean_tail_skipped_gflops over the step's GFLOPs).  The results go to OUT.json
(profiles/rellayers_cost.json).  usage: rellayers_cost.py [OUT.json]"""
import json
import os
import statistics as st
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import devit_amd  # noqa: E402
from devit_amd import engine  # noqa: E402

dev = torch.device("cuda")
B, C, ROUNDS, ITERS = 256, 25, 4, 4
CONFIGS = ("mid", "last", "all")
torch.manual_seed(0)
student = devit_amd.create_model("dedeit", num_classes=C, drop_path_rate=0.1).to(dev).train()
teacher = devit_amd.create_model("deit_base_distilled_patch16_224", num_classes=C).to(dev).eval()
for p in teacher.parameters():
    p.requires_grad_(False)
img = torch.randn(B, 3, 224, 224, device=dev)
soft = torch.nn.functional.one_hot(torch.randint(0, C, (B,), device=dev), C).float() * 0.9 + 0.1 / C


def step(sel):
    engine.distill_forward(student, teacher, img, soft, relation_layers=sel)["loss"].backward()


def sample(sel):
    for p in student.parameters():
        p.grad = None
    step(sel)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(ITERS):
        step(sel)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / ITERS


samples = {k: [] for k in CONFIGS}
for k in CONFIGS:
    sample(k)                           # first calls (allocator, module load) are not samples
for _ in range(ROUNDS):
    for k in CONFIGS:
        samples[k].append(round(sample(k), 3))
res = {"dekd_fwd_bwd_ms": {k: dict(samples=v, median=round(st.median(v), 3)) for k, v in samples.items()}}
base = res["dekd_fwd_bwd_ms"]["mid"]["median"]
res["ms_over_mid"] = {k: round(res["dekd_fwd_bwd_ms"][k]["median"] - base, 3) for k in ("last", "all")}
res["ratio_vs_mid"] = {k: round(res["dekd_fwd_bwd_ms"][k]["median"] / base, 4) for k in ("last", "all")}
res["estimates"] = {"all_ms_over_mid": round(11 * 0.24, 2), "all_note": "eleven more relation forward + backward pairs at 0.24 ms each",
                    "last_ratio_vs_mid": 1.068, "last_note": "the lean tail skips 6.8 % of the step's FLOPs; `last` runs both last blocks in full"}
res["shape"] = dict(B=B, N=198, student="dedeit", teacher="deit_base_distilled_patch16_224", rounds=ROUNDS, iters_per_sample=ITERS)
txt = json.dumps(res, indent=1)
print(txt)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write(txt + "\n")
