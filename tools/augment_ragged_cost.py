#!/usr/bin/env python3
"""What the packed-set form of the input stage costs (results: profiles/augment_ragged_cost.json).  The method is
tools/augment_cost.py's: bs 256, S = 224, bicubic, pixel-mode erasing on; warm = median of back-to-back calls, cold = median of calls that
each follow a 512 MB fill.

    augment_ragged_cost.py kernels [--batch-size 256] [--reps 40]
        (a) the uniform kernel (devit_augment_batch) on a 32 x 32 set against devit_augment_ragged on the same images packed, the same indices
            and table, ALTERNATING call by call: the price of the directory lookup, beside the spread of the uniform kernel's own repeats
        (b) a packed set of 375 x 500 images: the narrow kernel throughout
        (c) the same set with 5 % of the images at 1200 x 1600: both kernels run.  The wide kernel's share is measured by difference: the same
            call with the wide samples' rows replaced by an 8 x 8 crop of the same image (the wide kernel is still launched and every one of its
            workgroups leaves at once; the narrow kernel gets those 5 % as nearly free samples)
        (e) the host's draws + table validation per batch, on (c)'s sizes and on the uniform set
    augment_ragged_cost.py step --source ragged|synthetic [--steps 30] [--warmup 8]
        (d) augment_cost.py's DEKD step, fed by a DeviceLoader over set (c) or by resident random batches: run the two alternately
One JSON line on stdout."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def photo_set(dev, n, big_share, classes=25, seed=0):
    """a packed set of n random-byte images of 375 x 500, every 1 / big_share-th one 1200 x 1600 instead"""
    from devit_amd import data
    sizes = [(1200, 1600) if big_share and i % round(1 / big_share) == 0 else (375, 500) for i in range(n)]
    entries = np.zeros(n, dtype=data.IMAGE_ENTRY_DTYPE)
    at = 0
    for i, (h, w) in enumerate(sizes):
        entries[i] = (at, h, w)
        at += (3 * h * w + 15) // 16 * 16
    arena = np.random.default_rng(seed).integers(0, 256, at, dtype=np.uint8)
    return data.DeviceImageSet.from_packed(arena, entries, np.arange(n) % classes, [str(c) for c in range(classes)], dev)


def kernels(args):
    from devit_amd import data
    dev = torch.device("cuda")
    B, S = args.batch_size, 224
    g = torch.Generator().manual_seed(0)
    flush = torch.empty(512 << 20, dtype=torch.uint8, device=dev)
    out = torch.empty((B, 3, S, S), device=dev)
    kw = dict(interpolation='bicubic', re_prob=1.0, re_mode='pixel', seed=0)

    def once(fn, cold):
        if cold:
            flush.fill_(1)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    def stats(ms):
        return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}

    def timed(fns, cold):
        """the calls of fns alternating, args.reps rounds -> one stats dict per call"""
        for fn in fns:
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        ms = [[] for _ in fns]
        for _ in range(args.reps):
            for k, fn in enumerate(fns):
                ms[k].append(once(fn, cold))
        return [stats(m) for m in ms]

    def ragged_call(ds, idx, tab):
        sizes = ds.sizes[idx.cpu().numpy()]
        T = data.check_table(tab, sizes[:, 0], sizes[:, 1], S)
        tab_dev = data.upload(tab.view(np.uint8).reshape(-1), dev)
        return (lambda: data.augment_ragged(ds, idx, tab, S, seed=0, out=out, table_dev=tab_dev, max_taps=T)), T

    res = {"what": "kernels", "batch": B, "S": S, "filter": "bicubic", "erase": "pixel, re_prob 1", "reps": args.reps}
    # (a) the directory lookup
    imgs = torch.randint(0, 256, (50000, 32, 32, 3), generator=g, dtype=torch.uint8)
    uni = data.DeviceImageSet.from_arrays(imgs, torch.zeros(50000, dtype=torch.long), device=dev)
    packed = data.DeviceImageSet.from_arrays(imgs, torch.zeros(50000, dtype=torch.long), device=dev, ragged=True)
    idx = torch.randint(0, 50000, (B,), generator=g, dtype=torch.int32).to(dev)
    tab = data.TrainAugment(S, **kw).draw(B, 32, 32)
    tab_dev = data.upload(tab.view(np.uint8).reshape(-1), dev)
    uniform = lambda: data.augment_batch(uni.images, idx, tab, S, seed=0, out=out, table_dev=tab_dev)      # noqa: E731
    narrow, T = ragged_call(packed, idx, tab)
    ref = uniform().clone()
    assert torch.equal(ref, narrow()), "the packed path differs from the uniform one on the same images"
    res["a_directory_lookup"] = {"source": "50000 x 32x32", "max_taps": T}
    for name, cold in (("warm", False), ("cold", True)):
        u1, r, u2 = timed((uniform, narrow, uniform), cold)
        res["a_directory_lookup"][name] = {"uniform": u1, "ragged_narrow": r, "uniform_again": u2,
                                           "ragged_minus_uniform_ms": round(r["median_ms"] - (u1["median_ms"] + u2["median_ms"]) / 2, 4),
                                           "uniform_spread_ms": round(abs(u1["median_ms"] - u2["median_ms"]), 4)}
    del uni, packed, imgs
    # (b) photographs, narrow throughout; (c) 5 % large ones
    for key, share in (("b_375x500", 0.0), ("c_5pct_1200x1600", 0.05)):
        ds = photo_set(dev, 400, share)
        idx_h = torch.randint(0, 400, (B,), generator=g, dtype=torch.int32)
        if share:
            idx_h[:int(B * share)] = torch.arange(0, 400, round(1 / share))[torch.randint(0, 20, (int(B * share),), generator=g)].int()      # 5 % of the batch too
        idx = idx_h.to(dev)
        sizes = ds.sizes[idx_h.numpy()]
        tf = data.TrainAugment(S, **kw)
        tab = tf.draw(B, sizes[:, 0], sizes[:, 1])
        call, T = ragged_call(ds, idx, tab)
        wide = np.maximum(data.taps_bound(tab["h"], S, tab["filter"]), data.taps_bound(tab["w"], S, tab["filter"])) > 12
        entry = {"arena_bytes": int(ds.arena.shape[0]), "max_taps": T, "wide_samples": int(wide.sum()), "big_images_in_batch": int((sizes[:, 0] == 1200).sum())}
        fns = [call]
        if share:
            small = tab.copy()
            small["h"][wide], small["w"][wide] = 8, 8
            small_dev = data.upload(small.view(np.uint8).reshape(-1), dev)
            fns.append(lambda: data.augment_ragged(ds, idx, small, S, seed=0, out=out, table_dev=small_dev, max_taps=T))
        for name, cold in (("warm", False), ("cold", True)):
            t = timed(fns, cold)
            entry[name] = t[0]
            if share:
                entry[name + "_wide_rows_made_small"] = t[1]
                entry[name + "_wide_kernel_share"] = round(1 - t[1]["median_ms"] / t[0]["median_ms"], 3)
        if share:                                              # (e) the host: draws + validation per batch
            t0 = time.perf_counter()
            for _ in range(20):
                tb = tf.draw(B, sizes[:, 0], sizes[:, 1])
            t1 = time.perf_counter()
            for _ in range(20):
                data.check_table(tb, sizes[:, 0], sizes[:, 1], S)
            t2 = time.perf_counter()
            uni_tf = data.TrainAugment(S, **kw)
            for _ in range(20):
                uni_tf.draw(B, 32, 32)
            t3 = time.perf_counter()
            res["e_host_ms_per_batch"] = {"draw_mixed_sizes": round((t1 - t0) / 20 * 1e3, 3), "check_table_ragged": round((t2 - t1) / 20 * 1e3, 3),
                                          "draw_uniform_32x32": round((t3 - t2) / 20 * 1e3, 3)}
        res[key] = entry
        del ds
    print(json.dumps(res))


def step(args):
    import augment_cost as AC
    import devit_amd
    import distill_sub
    from devit_amd import data, ddp, engine, losses, optim
    dev = torch.device("cuda")
    B, C, n = args.batch_size, 25, args.warmup + args.steps
    torch.manual_seed(0)
    student = devit_amd.create_model("dedeit", num_classes=C, drop_path_rate=0.1, drop_block_rate=None).to(dev).train()
    torch.manual_seed(1)
    teacher = devit_amd.create_model("deit_base_distilled_patch16_224", num_classes=C).to(dev).eval()
    for p in teacher.parameters():
        p.requires_grad_(False)
    teacher.request_precision("bf16")
    flat = ddp.FlatParams(student)
    ddp.broadcast_parameters(flat)
    flat.attach_bf16(student)
    reducer = ddp.BucketedGradReducer(flat).attach(student)
    opt = optim.FlatAdamW(flat, lr=5e-4 * B / 512.0, weight_decay=0.0, max_norm=1.0, ema_decay=0.99996)
    criterion = losses.DistillLoss(losses.SoftTargetCrossEntropy(), "hard", 0.5, 1.0)
    g = torch.Generator(device=dev).manual_seed(1234)
    y1, y2 = (torch.randint(0, C, (B,), generator=g, device=dev) for _ in range(2))
    oh = lambda y: torch.full((B, C), 0.1 / C, device=dev).scatter_(1, y[:, None], 0.9 + 0.1 / C)      # noqa: E731
    soft = 0.7 * oh(y1) + 0.3 * oh(y2)
    if args.source == "ragged":
        ds = photo_set(dev, 400, 0.05, C)
        sampler = torch.randint(0, 400, (n * B,), generator=torch.Generator().manual_seed(0)).tolist()
        loader = data.DeviceLoader(ds, sampler, B, data.TrainAugment(224, re_prob=0.25, re_mode='pixel', seed=0), drop_last=True)
    else:
        loader = distill_sub.SyntheticLoader(n, B, C, dev, 1234)
    look = engine.TeacherLookahead(teacher)
    batches = engine._PreparedBatches(AC._SoftTargets(loader, soft), dev, None, look, row_dtypes=engine.row_dtypes_for(student, teacher))
    feed = iter(batches)
    start_flat, start_flat16 = flat.flat.clone(), flat.flat16.clone()

    def one():
        flat.flat.copy_(start_flat)
        flat.flat16.copy_(start_flat16)
        flat.refresh_kmajor()
        opt.zero_grad()
        x, y, t_out = next(feed)
        out = engine.distill_forward(student, teacher, x, y, gama=(0.2, 0.1, 0.3), criterion=criterion, teacher_outputs=t_out,
                                     after_student=batches.launch_teacher)
        out["loss"].backward()
        reducer.finish()
        opt.step()
        return out["loss"]
    for _ in range(args.warmup):
        one()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        loss = one()
    t_enqueue = time.perf_counter() - t0
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assert bool(torch.isfinite(loss)), "non-finite loss"
    print(json.dumps({"what": "step", "source": args.source, "batch": B, "steps": args.steps, "warmup": args.warmup,
                      "value": round(B * args.steps / dt, 1), "unit": "images/sec", "step_ms": round(dt / args.steps * 1e3, 3),
                      "host_enqueue_ms_per_step": round(t_enqueue / args.steps * 1e3, 3), "loss": float(loss)}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("what", choices=["kernels", "step"])
    ap.add_argument("--source", default="ragged", choices=["ragged", "synthetic"])
    ap.add_argument("--batch-size", type=int, default=256)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--reps", type=int, default=40)
    a = ap.parse_args()
    (kernels if a.what == "kernels" else step)(a)
