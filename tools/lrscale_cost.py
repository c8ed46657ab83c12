#!/usr/bin/env python3
"""What the learning rate per granule costs the AdamW tail: devit_adamw_step_lrs against devit_adamw_step on the same buffers, at the student's flat
size (dedeit) and at DeiT-B's, with weight decay 0.05 over timm's two groups, the clip at 1.0, EMA and the bf16 copy on, and the group bytes and
table --layer-decay 0.75 builds.  Cold cache (the Infinity Cache is flushed before every launch), rounds that alternate the two entry points in one
process (the order within a round alternates too), median and range of each one's samples; `same`: the unscaled entry point against itself in the
same rounds, which is the spread a ratio has to leave before it means anything.  The learning rate is 0, so the buffers keep their values.
usage: lrscale_cost.py [OUT.json]"""
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
ROUNDS, SEED, DECAY = 15, 20261021, 0.75
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


def measure(name):
    torch.manual_seed(SEED)
    model = devit_amd.create_model(name, num_classes=25).to(dev)
    flat = ddp.FlatParams(model).attach_bf16(model)
    flat.flat_grad.copy_(torch.randn(flat.numel, generator=torch.Generator(device=dev).manual_seed(SEED), device=dev) * 1e-3)
    depth = optim.model_depth(model)
    o = optim.FlatAdamW(flat, lr=0.0, weight_decay=0.05, max_norm=1.0, ema_decay=0.99996, no_decay=optim.no_decay_names(model),
                        lr_scales=optim.layer_decay_scales(flat.names, depth, DECAY))
    o.step()          # one whole step: the norm, the scalars in `dyn`, module load
    f, n = flat, flat.numel
    args = (ptr(f.flat), ptr(f.flat_grad), ptr(o.m), ptr(o.v), ptr(o.ema), ptr(f.flat16), ptr(o.no_decay4), ptr(o.gnorm_sq), ptr(o._dyn), n,
            o.betas[0], o.betas[1], o.eps, o.weight_decay, float(o.max_norm), float(o.ema_decay), 1.0)
    plain = lambda: call("devit_adamw_step", *args, stream_ptr())
    scaled = lambda: call("devit_adamw_step_lrs", *args, ptr(o.lr_group4), ptr(o.lr_scales), stream_ptr())
    kernels = {"unscaled": plain, "scaled": scaled, "same": plain}
    for fn in kernels.values():
        fn()
    torch.cuda.synchronize()
    samples = {k: [] for k in kernels}
    for r in range(ROUNDS):
        order = list(kernels) if r % 2 == 0 else list(kernels)[::-1]
        for k in order:
            samples[k].append(cold(kernels[k]))
    res = {k: dict(us_median=round(st.median(v), 1), us_min=round(min(v), 1), us_max=round(max(v), 1)) for k, v in samples.items()}
    med = lambda k: st.median(samples[k])
    bytes_per_granule = 4 * (16 + 4 + 18) + 1          # p, g, m, v, ema read; p, m, v, ema, bf16 written; the no_decay4 byte
    res.update(elements=n, groups=depth + 2, bytes_per_granule_unscaled=bytes_per_granule, bytes_per_granule_scaled=bytes_per_granule + 1,
               gb_per_s_unscaled=round(bytes_per_granule * (n // 4) / med("unscaled") / 1e3, 1),
               scaled_over_unscaled=round(med("scaled") / med("unscaled"), 4), same_over_unscaled=round(med("same") / med("unscaled"), 4),
               per_round_ratio_min_max=[round(min(s / u for s, u in zip(samples["scaled"], samples["unscaled"])), 4),
                                        round(max(s / u for s, u in zip(samples["scaled"], samples["unscaled"])), 4)])
    return res


out = {name: measure(name) for name in ("dedeit", "deit_base_patch16_224")}
out["shape"] = dict(rounds=ROUNDS, cache="cold", layer_decay=DECAY, weight_decay=0.05, clip=1.0, ema=True, bf16_copy=True)
txt = json.dumps(out, indent=1)
print(txt)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as fh:
        fh.write(txt + "\n")
