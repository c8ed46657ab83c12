#!/usr/bin/env python3
"""What the optimizer tails cost next to AdamW's at dedeit's flat size (21.7 M elements; weight decay 0.05 with timm's two groups, clip at 1.0, EMA
and the bf16 copy on): cold-cache launches (Infinity Cache flushed before each), rounds that alternate the five tails, median and range of each
one's samples.  Timed: the optimizer entry point alone (devit_adamw_step, devit_sgd_step x 2, devit_adam_l2_step, devit_lamb_step's three launches);
the norm (devit_sumsq_f32) and the k-major refresh are the same for all and stay outside.
usage: opt_step_cost.py [OUT.json]"""
import json
import os
import statistics as st
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import devit_amd  # noqa: E402
from devit_amd import ddp, optim  # noqa: E402
from devit_amd._lib import call, ptr, stream_ptr  # noqa: E402

dev = torch.device("cuda")
ROUNDS, SEED = 9, 20241019
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


torch.manual_seed(SEED)
model = devit_amd.create_model("dedeit", num_classes=25).to(dev)
flat = ddp.FlatParams(model).attach_bf16(model)
flat.flat_grad.copy_(torch.randn(flat.numel, generator=torch.Generator(device=dev).manual_seed(SEED), device=dev) * 1e-3)
kw = dict(lr=1e-6, weight_decay=0.05, max_norm=1.0, ema_decay=0.99996, no_decay=optim.no_decay_names(model))
opts = {"adamw": optim.FlatAdamW(flat, **kw), "momentum": optim.FlatSGD(flat, **kw), "nesterov": optim.FlatSGD(flat, nesterov=True, **kw),
        "adam": optim.FlatAdam(flat, **kw), "lamb": optim.FlatLamb(flat, **kw)}
for o in opts.values():          # one whole step each: the norm, the scalars in `dyn`, module load
    o.step()
torch.cuda.synchronize()
f, n = flat, flat.numel


def launch(name):
    o = opts[name]
    common = (o.weight_decay, float(o.max_norm), float(o.ema_decay), 1.0, stream_ptr())
    if name in ("adamw", "adam"):
        return lambda: call("devit_adamw_step" if name == "adamw" else "devit_adam_l2_step", ptr(f.flat), ptr(f.flat_grad), ptr(o.m), ptr(o.v), ptr(o.ema),
                            ptr(f.flat16), ptr(o.no_decay4), ptr(o.gnorm_sq), ptr(o._dyn), n, o.betas[0], o.betas[1], o.eps, *common)
    if name == "lamb":
        return lambda: call("devit_lamb_step", ptr(f.flat), ptr(f.flat_grad), ptr(o.m), ptr(o.v), ptr(o.ema), ptr(f.flat16), ptr(o.gnorm_sq), ptr(o._dyn), n,
                            ptr(o.chunks), o.nchunks, o.nsegments, 0, o.betas[0], o.betas[1], o.eps, *common[:4], ptr(o._lamb_ws), o._lamb_ws.numel(),
                            stream_ptr())
    return lambda: call("devit_sgd_step", ptr(f.flat), ptr(f.flat_grad), ptr(o.buf), ptr(o.ema), ptr(f.flat16), ptr(o.no_decay4), ptr(o.gnorm_sq),
                        ptr(o._dyn), n, o.momentum, int(o.nesterov), *common)


# algorithmic bytes per element, EMA and bf16 copy included: read + written
BYTES = {"adamw": 16 + 4 + 18, "adam": 16 + 4 + 18, "momentum": 12 + 4 + 14, "nesterov": 12 + 4 + 14, "lamb": (16 + 8) + (12 + 4 + 10)}
kernels = {k: launch(k) for k in opts}
samples = {k: [] for k in kernels}
for _ in range(ROUNDS):
    for k, fn in kernels.items():
        samples[k].append(cold(fn))
res = {k: dict(us_median=round(st.median(v), 1), us_min=round(min(v), 1), us_max=round(max(v), 1), bytes_per_element=BYTES[k],
               gb_per_s=round(BYTES[k] * n / st.median(v) / 1e3, 1)) for k, v in samples.items()}
res["ratios"] = {f"{k} / adamw": round(res[k]["us_median"] / res["adamw"]["us_median"], 3) for k in kernels if k != "adamw"}
res["shape"] = dict(model="dedeit", elements=n, rounds=ROUNDS, cache="cold", lamb_chunks=opts["lamb"].nchunks, lamb_tensors=opts["lamb"].nsegments)
txt = json.dumps(res, indent=1)
print(txt)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as fh:
        fh.write(txt + "\n")
