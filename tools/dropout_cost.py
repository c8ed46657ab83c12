#!/usr/bin/env python3
"""What the dropout kernels cost at the student's shapes (B = 256, N = 198, D = 384, H = 6, hidden 1536), next to their p == 0 siblings and the
bytes they move: cold-cache launches (Infinity Cache flushed before each), five rounds that alternate plain and dropout kernels, median of
each kernel's samples.  The passes (devit_dropout_apply / _residual) are extra launches of a p > 0 block; the attention kernels replace
devit_attn_fwd / _bwd.  usage: dropout_cost.py [OUT.json]"""
import json
import os
import statistics as st
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from devit_amd import dropout, ops  # noqa: E402
from devit_amd._lib import call, ptr, stream_ptr  # noqa: E402

dev = torch.device("cuda")
BF16, F32 = torch.bfloat16, torch.float32
B, N, H, D, HID = 256, 198, 6, 384, 1536
M, SEED, ROUNDS = B * N, 20240807, 5
flush = torch.empty(320 << 20, dtype=torch.uint8, device=dev)


def cold(fn):
    flush.zero_()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3


def rnd(rows, cols, dtype):
    t = ops.rows_alloc(rows, cols, dtype, dev)
    t[:rows] = torch.randn(rows, cols, device=dev).to(dtype)
    return t


h, g, colsum = rnd(M, HID, BF16), rnd(M, D, BF16), torch.zeros(D, device=dev)
x, y, dp = torch.randn(M, D, device=dev), torch.randn(M, D, device=dev), torch.ones(B, device=dev)
qkv, dout = rnd(M, 3 * D, BF16), rnd(M, D, BF16)
out, lse, dqkv = ops.rows_alloc(M, D, BF16, dev), torch.empty(B, H, N, device=dev), ops.rows_alloc(M, 3 * D, BF16, dev)
thr, s = dropout.threshold(0.1)
st_ = stream_ptr

kernels = {
    # name: (launch, algorithmic bytes)
    "apply_bf16_hidden": (lambda: dropout.apply_(h, M, SEED, 3, 0, 0.1), 2 * M * HID * 2),
    "apply_bf16_D_colsum": (lambda: dropout.apply_(g, M, SEED, 4, 0, 0.1, colsum=colsum), 2 * M * D * 2),
    "residual_f32_D": (lambda: dropout.residual(x, y, dp, N, SEED, 2, 0, 0.1, out=x), 3 * M * D * 4),
    "attn_fwd": (lambda: call("devit_attn_fwd", ptr(qkv), ptr(out), ptr(lse), None, B, N, H, 64, 0.125, 0, st_()), 4 * M * D * 2),
    "attn_fwd_drop": (lambda: call("devit_attn_fwd_drop", ptr(qkv), ptr(out), ptr(lse), None, B, N, H, 64, 0.125, SEED, 0, thr, s, st_()),
                      4 * M * D * 2),
    "attn_bwd": (lambda: call("devit_attn_bwd", ptr(qkv), ptr(out), ptr(dout), ptr(lse), None, None, ptr(dqkv), B, N, H, 64, 0.125, st_()),
                 8 * M * D * 2),
    "attn_bwd_drop": (lambda: call("devit_attn_bwd_drop", ptr(qkv), ptr(out), ptr(dout), ptr(lse), None, None, ptr(dqkv), B, N, H, 64, 0.125,
                                   SEED, 0, thr, s, st_()), 8 * M * D * 2),
}
for fn, _ in kernels.values():      # first launches (module load, attribute calls) are not samples
    fn()
samples = {k: [] for k in kernels}
for _ in range(ROUNDS):
    for k, (fn, _) in kernels.items():
        samples[k].append(cold(fn))
res = {k: dict(us_median=round(st.median(v), 1), us_min=round(min(v), 1), us_max=round(max(v), 1), bytes=kernels[k][1],
               gb_per_s=round(kernels[k][1] / st.median(v) / 1e3, 1)) for k, v in samples.items()}
res["ratios"] = {"attn_fwd_drop / attn_fwd": round(res["attn_fwd_drop"]["us_median"] / res["attn_fwd"]["us_median"], 2),
                 "attn_bwd_drop / attn_bwd": round(res["attn_bwd_drop"]["us_median"] / res["attn_bwd"]["us_median"], 2)}
res["shape"] = dict(B=B, N=N, H=H, D=D, hidden=HID, p=0.1, rounds=ROUNDS, cache="cold")
txt = json.dumps(res, indent=1)
print(txt)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write(txt + "\n")
