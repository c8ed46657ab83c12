#!/usr/bin/env python3
"""What --hid-gama costs in the step: the DEKD step's forward + backward (student + teacher + losses; the optimizer does not depend on it) at bs 256
with hid_gama 0 and 0.3, five rounds that alternate the two configurations on one box, each sample the mean of ITERS iterations between two events.
The ratio against hid_gama 0 goes to OUT.json (profiles/hid_step_cost.json).  usage: hid_step_cost.py [OUT.json]"""
import json
import os
import statistics as st
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import devit_amd  # noqa: E402
from devit_amd import engine  # noqa: E402

dev = torch.device("cuda")
B, C, ROUNDS, ITERS = 256, 25, 5, 4
CONFIGS = {"hid_gama0": 0.0, "hid_gama0.3": 0.3}
torch.manual_seed(0)
student = devit_amd.create_model("dedeit", num_classes=C, drop_path_rate=0.1).to(dev).train()
teacher = devit_amd.create_model("deit_base_distilled_patch16_224", num_classes=C).to(dev).eval()
for p in teacher.parameters():
    p.requires_grad_(False)
img = torch.randn(B, 3, 224, 224, device=dev)
soft = torch.nn.functional.one_hot(torch.randint(0, C, (B,), device=dev), C).float() * 0.9 + 0.1 / C


def step(g):
    engine.distill_forward(student, teacher, img, soft, hid_gama=g)["loss"].backward()


def sample(g):
    for p in student.parameters():
        p.grad = None
    step(g)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(ITERS):
        step(g)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / ITERS


samples = {k: [] for k in CONFIGS}
for g in CONFIGS.values():
    sample(g)                           # first calls (allocator, module load) are not samples
for _ in range(ROUNDS):
    for k, g in CONFIGS.items():
        samples[k].append(round(sample(g), 3))
res = {"dekd_fwd_bwd_ms": {k: dict(samples=v, median=round(st.median(v), 3)) for k, v in samples.items()}}
res["ratio_vs_hid_gama0"] = round(res["dekd_fwd_bwd_ms"]["hid_gama0.3"]["median"] / res["dekd_fwd_bwd_ms"]["hid_gama0"]["median"], 4)
res["shape"] = dict(B=B, N=198, student_width=384, teacher_width=768, layer_pair=[5, 5], rounds=ROUNDS, iters_per_sample=ITERS)
txt = json.dumps(res, indent=1)
print(txt)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write(txt + "\n")
