#!/usr/bin/env python3
"""What dropout p > 0 costs in the step: the student's forward + backward at bs 256 and the DEKD step's forward + backward (student + teacher +
losses; the optimizer does not depend on p), for p = 0, drop_rate = 0.1 and attn_drop_rate = 0.1, five rounds that alternate the three
configurations on one box, each sample the mean of ITERS iterations between two events.  Ratios against p = 0 and the bytes the extra passes
move go to OUT.json.  usage: dropout_step_cost.py [OUT.json]"""
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
CONFIGS = {"p0": dict(), "drop0.1": dict(drop_rate=0.1), "attn_drop0.1": dict(attn_drop_rate=0.1)}
torch.manual_seed(0)
students = {k: devit_amd.create_model("dedeit", num_classes=C, drop_path_rate=0.1, **kw).to(dev).train() for k, kw in CONFIGS.items()}
for m in list(students.values())[1:]:
    m.load_state_dict(students["p0"].state_dict())
teacher = devit_amd.create_model("deit_base_distilled_patch16_224", num_classes=C).to(dev).eval()
img = torch.randn(B, 3, 224, 224, device=dev)
soft = torch.nn.functional.one_hot(torch.randint(0, C, (B,), device=dev), C).float() * 0.9 + 0.1 / C


def student_fb(m):
    lo, lk = m(img)
    (lo.sum() + lk.sum()).backward()


def dekd_fb(m):
    engine.distill_forward(m, teacher, img, soft)["loss"].backward()


def sample(fn, m):
    for p in m.parameters():
        p.grad = None
    fn(m)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(ITERS):
        fn(m)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / ITERS


res = {}
for name, fn in (("student_fwd_bwd_ms", student_fb), ("dekd_fwd_bwd_ms", dekd_fb)):
    samples = {k: [] for k in CONFIGS}
    for k, m in students.items():
        sample(fn, m)                   # first calls (allocator, module load) are not samples
    for _ in range(ROUNDS):
        for k, m in students.items():
            samples[k].append(round(sample(fn, m), 3))
    res[name] = {k: dict(samples=v, median=round(st.median(v), 3)) for k, v in samples.items()}
    res[name]["ratio_vs_p0"] = {k: round(res[name][k]["median"] / res[name]["p0"]["median"], 3) for k in CONFIGS if k != "p0"}
M, D, HID, NB = B * 198, 384, 1536, 12
Mp = (M + 255) // 256 * 256
res["extra_bytes_per_step_drop0.1"] = dict(
    forward=NB * (2 * M * HID * 2 + 2 * (3 * M * D * 4)), backward=NB * (2 * M * HID * 2 + 2 * (2 * M * D * 2)),
    note="per block: apply on the hidden (read + write bf16) and two residual passes (x, y in, x out, fp32) forward; apply on dh_pre and on g2 / g1 backward; "
         "the residual passes replace the GEMM epilogue's read of x, so their net cost is the fp32 temporary's write + read")
res["shape"] = dict(B=B, N=198, D=D, hidden=HID, blocks=NB, rounds=ROUNDS, iters_per_sample=ITERS)
txt = json.dumps(res, indent=1)
print(txt)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write(txt + "\n")
