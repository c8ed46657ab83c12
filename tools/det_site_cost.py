#!/usr/bin/env python3
"""Deterministic mode, per site: the ordered reduction at the default path's slice count against the same entry point with ONE slice (split_k = 1:
no partial sums to order), on the step's shapes at bs 256 -- the four weight gradients of a student (D = 384) and a teacher-sized (D = 768) block
and the patch embedding on the split-K 128 x 128 launches, one block and eleven blocks on the grouped full-row kernel.  Per row, microseconds per
launch (median of REPEATS samples of ITERS back-to-back launches): the default mode at its slice count (the atomics), deterministic mode at the same
count (partials + fold), and one slice.  `verdict` says which of the last two deterministic mode should take.
usage: det_site_cost.py [OUT.json]   (profiles/det_site_cost.json)"""
import json
import os
import statistics as st
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from devit_amd import _lib as L, ops  # noqa: E402

dev = torch.device("cuda")
MP, REPEATS, ITERS = 256 * 198, 3, 10           # 50688 token rows = 792 K-steps
BF16, F32 = torch.bfloat16, torch.float32


def timed(fn):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(REPEATS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(ITERS):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / ITERS)
    return round(st.median(out), 1)


def three(launch, split):
    """launch(split_k) under: default mode at `split`, deterministic mode at `split`, one slice"""
    with ops.deterministic(False):
        a = timed(lambda: launch(split))
    with ops.deterministic(True):
        d = timed(lambda: launch(split))
        one = timed(lambda: launch(1))
    return dict(default_us=a, det_us=d, one_slice_us=one, det_vs_default=round(d / a, 3), verdict="ordered split" if d <= one else "one slice")


rows = []
g = torch.Generator(device="cpu").manual_seed(0)
for label, shapes in (("student block (D 384)", (("qkv", 1152, 384), ("proj", 384, 384), ("fc1", 1536, 384), ("fc2", 384, 1536))),
                      ("teacher-sized block (D 768)", (("qkv", 2304, 768), ("proj", 768, 768), ("fc1", 3072, 768), ("fc2", 768, 3072))),
                      ("patch embedding", (("D384", 384, 768), ("D768", 768, 768)))):
    for name, N, K in shapes:
        dy = (torch.randn(MP, N, generator=g) * 0.05).to(BF16).to(dev)
        x = torch.randn(MP, K, generator=g).to(BF16).to(dev)
        wg, bg = torch.zeros(N, K, device=dev), torch.zeros(N, device=dev)
        split = ops.split_k_for(N, K, MP // 64)
        r = three(lambda sk: ops.gemm(dy, N, 1, x, K, 1, N, K, MP, kind=L.EPI_ATOMIC_F32, out=wg, ldc=K, split_k=sk, aux=bg), split)
        rows.append(dict(site="devit_gemm_bf16 ATOMIC_F32", what=f"{label}: {name} [{N} x {K}]", split_k=split, **r))
        print(rows[-1], flush=True)
        del dy, x

# the grouped full-row kernel: a student block's four products as jobs, one block and eleven
D, H = 384, 1536
acts = dict(dqkv=(MP, 3 * D), ln1=(MP, D), dattn=(MP, D), attn=(MP, D), dh=(MP, H), ln2=(MP, D), g2=(MP, D), h=(MP, H))
t = {k: (torch.randn(s, generator=g) * 0.05).to(BF16).to(dev) for k, s in acts.items()}
for blocks in (1, 11):
    jobs, keep = [], []
    for _ in range(blocks):
        for dy, x, n, k in ((t["dqkv"], t["ln1"], 3 * D, D), (t["dattn"], t["attn"], D, D), (t["dh"], t["ln2"], H, D), (t["g2"], t["h"], D, H)):
            w = torch.zeros(n, k, device=dev)
            b = torch.zeros(n, device=dev) if k == D else None
            keep += [w, b]
            jobs.append(ops.wgrad_job_struct(dy, x, w, b))
    arr = (L.WgradJob * len(jobs))(*jobs)
    r = three(lambda sk: ops.call("devit_wgrad_grouped", arr, len(jobs), MP, sk, L.stream_ptr()), 0)
    rows.append(dict(site="devit_wgrad_grouped", what=f"{blocks} student block(s), {len(jobs)} jobs", split_k="cost model (13 for one block, 1 for eleven)", **r))
    print(rows[-1], flush=True)

txt = json.dumps(dict(rows=rows, token_rows=MP, repeats=REPEATS, iters_per_sample=ITERS), indent=1)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write(txt + "\n")
