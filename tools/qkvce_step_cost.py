#!/usr/bin/env python3
"""What --qkv-ce-gama / --qkv-cross-gama cost in the step: the DEKD step's forward + backward (student + teacher + losses; the optimizer does not depend
on them) at bs 256 with both weights 0, the self mode alone and the cross mode alone, five rounds that alternate the three configurations on one box,
each sample the mean of ITERS iterations between two events; and the cold times of the new kernels on the step's shapes (one call between two events
behind a cache-sized memset, the median of nine).  The results go to OUT.json (profiles/qkvce_step_cost.json).  usage: qkvce_step_cost.py [OUT.json]"""
import json
import os
import statistics as st
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import devit_amd  # noqa: E402
from devit_amd import engine, ops  # noqa: E402
from devit_amd._lib import ptr, stream_ptr  # noqa: E402

dev = torch.device("cuda")
B, C, ROUNDS, ITERS = 256, 25, 5, 4
CONFIGS = {"weights0": (0.0, 0.0), "self0.3": (0.3, 0.0), "cross0.3": (0.0, 0.3)}
torch.manual_seed(0)
student = devit_amd.create_model("dedeit", num_classes=C, drop_path_rate=0.1).to(dev).train()
teacher = devit_amd.create_model("deit_base_distilled_patch16_224", num_classes=C).to(dev).eval()
for p in teacher.parameters():
    p.requires_grad_(False)
img = torch.randn(B, 3, 224, 224, device=dev)
soft = torch.nn.functional.one_hot(torch.randint(0, C, (B,), device=dev), C).float() * 0.9 + 0.1 / C


def step(w):
    engine.distill_forward(student, teacher, img, soft, qkv_ce_gama=w[0], qkv_cross_gama=w[1])["loss"].backward()


def sample(w):
    for p in student.parameters():
        p.grad = None
    step(w)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(ITERS):
        step(w)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / ITERS


samples = {k: [] for k in CONFIGS}
for w in CONFIGS.values():
    sample(w)                           # first calls (allocator, module load) are not samples
for _ in range(ROUNDS):
    for k, w in CONFIGS.items():
        samples[k].append(round(sample(w), 3))
res = {"dekd_fwd_bwd_ms": {k: dict(samples=v, median=round(st.median(v), 3)) for k, v in samples.items()}}
base = res["dekd_fwd_bwd_ms"]["weights0"]["median"]
res["ratio_vs_weights0"] = {k: round(res["dekd_fwd_bwd_ms"][k]["median"] / base, 4) for k in ("self0.3", "cross0.3")}

# ---- the kernels alone, cold, on the step's shapes
N, Ds, Dt = 198, 384, 768
s_buf = ops.rows_alloc(B * N, 3 * Ds, torch.bfloat16, dev)
t_buf = ops.rows_alloc(B * N, 3 * Dt, torch.bfloat16, dev)
s_buf[: B * N].normal_(std=0.5)
t_buf[: B * N].normal_(std=0.5)
flush = torch.empty(512 << 20, dtype=torch.uint8, device=dev)
up = torch.ones(1, device=dev)


def cold(fn):
    out = []
    for _ in range(9):
        flush.zero_()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3)
    return round(st.median(out), 1)


kern = {}
for name, cross in (("self", 0), ("cross", 1)):
    P = 9 if cross else 3
    terms = torch.empty((P, B * N), device=dev)
    S = torch.empty((P, B, 208, 224), dtype=torch.bfloat16, device=dev)
    loss = torch.empty(1, device=dev)
    d = torch.empty_like(s_buf)
    fwd = lambda: ops.call("devit_qkv_pair_fwd", ptr(s_buf), ptr(t_buf), B, N, Ds, Dt, 3 * Ds, 3 * Dt, 64, 64, 0, cross, 0, 1, ptr(terms), ptr(S),  # noqa: E731
                           ptr(loss), stream_ptr())
    bwd = lambda: ops.call("devit_qkv_pair_bwd", ptr(S), ptr(s_buf), ptr(up), B, N, Ds, 3 * Ds, 64, cross, 0, ptr(d), 3 * Ds, stream_ptr())  # noqa: E731
    fwd()
    bwd()
    kern[name] = dict(fwd_us=cold(fwd), bwd_us=cold(bwd))
res["kernels_cold_us"] = kern
res["shape"] = dict(B=B, N=N, student_width=Ds, teacher_width=Dt, layer_pair=[5, 5], layout="view", rounds=ROUNDS, iters_per_sample=ITERS)
txt = json.dumps(res, indent=1)
print(txt)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write(txt + "\n")
