#!/usr/bin/env python3
"""What the per-sample Mixup / CutMix pass costs next to the batch-mode one at the step's shape (B = 256, bf16 rows only): cold-cache launches
(Infinity Cache flushed before each), rounds that alternate the three configurations, median and spread of each one's samples.
  batch_mode1:  devit_mix_im2row_bf16, mode 1 (every image read twice)
  table_mode1:  devit_mix_im2row_table with an all-mixup table: the same bytes plus the 8 KB table
  table_elem:   devit_mix_im2row_table with a table drawn by Mixup(mode='elem') at the default alphas: about half the samples are CutMix
                and read their partner only inside the box
usage: mix_table_cost.py [OUT.json]"""
import json
import os
import statistics as st
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from devit_amd import ops  # noqa: E402
from devit_amd._lib import call, ptr, stream_ptr  # noqa: E402
from distill_sub import Mixup  # noqa: E402

dev = torch.device("cuda")
B, ROUNDS, SEED = 256, 9, 20240807
IMG_BYTES, ROW_BYTES = B * 3 * 224 * 224 * 4, B * 196 * 768 * 2
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


img = torch.randn((B, 3, 224, 224), generator=torch.Generator(device=dev).manual_seed(SEED), device=dev)
rows = ops.rows_alloc(B * 196, 768, torch.bfloat16, dev)
all_mix = ops.mix_table([(1, 0.3, 0, 0, 0, 0)] * B, dev)
np.random.seed(SEED)
elem = ops.mix_table(Mixup(0.8, 1.0, 1.0, 0.5, 0.1, 25, mode="elem").draw_table(B), dev)


def partner_share(host):
    """share of the partner image a table's samples read: all of it for mixup, the 8-element chunks that meet the box for cutmix"""
    s = 0.0
    for e in host:
        if e["mode"] == 1:
            s += 1.0
        elif e["mode"] == 2 and e["y1"] > e["y0"] and e["x1"] > e["x0"]:
            s += (int(e["y1"]) - int(e["y0"])) * ((int(e["x1"]) + 7) // 8 - int(e["x0"]) // 8) * 8 / (224.0 * 224.0)
    return s / len(host)


def table_launch(t):
    return lambda: call("devit_mix_im2row_table", ptr(img), ptr(rows), None, None, ptr(t.dev), B, stream_ptr())


kernels = {
    # name: (launch, algorithmic bytes)
    "batch_mode1": (lambda: call("devit_mix_im2row_bf16", ptr(img), ptr(rows), None, B, 1, 0.3, 0, 0, 0, 0, stream_ptr()), 2 * IMG_BYTES + ROW_BYTES),
    "table_mode1": (table_launch(all_mix), 2 * IMG_BYTES + ROW_BYTES + all_mix.host.nbytes),
    "table_elem": (table_launch(elem), int((1 + partner_share(elem.host)) * IMG_BYTES) + ROW_BYTES + elem.host.nbytes),
}
for fn, _ in kernels.values():      # first launches (module load) are not samples
    fn()
samples = {k: [] for k in kernels}
for _ in range(ROUNDS):
    for k, (fn, _) in kernels.items():
        samples[k].append(cold(fn))
res = {k: dict(us_median=round(st.median(v), 1), us_min=round(min(v), 1), us_max=round(max(v), 1), bytes=kernels[k][1],
               gb_per_s=round(kernels[k][1] / st.median(v) / 1e3, 1)) for k, v in samples.items()}
res["ratios"] = {"table_mode1 / batch_mode1": round(res["table_mode1"]["us_median"] / res["batch_mode1"]["us_median"], 3),
                 "table_elem / batch_mode1": round(res["table_elem"]["us_median"] / res["batch_mode1"]["us_median"], 3)}
modes = elem.host["mode"]
res["shape"] = dict(B=B, rows="bf16", rounds=ROUNDS, cache="cold", elem_table=dict(none=int((modes == 0).sum()), mixup=int((modes == 1).sum()),
                                                                                  cutmix=int((modes == 2).sum()),
                                                                                  partner_share=round(partner_share(elem.host), 3)))
txt = json.dumps(res, indent=1)
print(txt)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write(txt + "\n")
