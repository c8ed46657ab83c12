#!/usr/bin/env python3
"""Headline benchmark: images/sec of one distill_sub optimisation step (DeiT-B -> dedeit, bs 256 per GPU,
224x224, bf16) -- BASELINE.json `metric`.

A step = zero grads, student train forward (output_qkv), teacher eval forward, DEKD losses, backward with the
bucketed RCCL gradient all-reduce, global-norm clip + AdamW + EMA + bf16 weight re-cast (engine.py:62-132 of
the reference).  Inputs are synthetic and already resident in HBM; weights are random-init, and every step starts
from them again (one copy of the fp32 masters and of their bf16 copy per step).

    python bench.py --gpus 1 --steps 20 --warmup 5
    python bench.py --gpus 1 --steps 20 --warmup 5 --full   (+ roofline, exchange, parity, CPU baseline)
    python bench.py --gpus 1 --steps 20 --warmup 5 --dump-outputs DIR
    python bench.py --gpus N ...            (no launcher: starts its own N ranks, one per GPU, before touching a GPU)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
           bench.py --gpus N --steps K --warmup W

Prints ONE JSON line (rank 0).  A plain run sets up, warms up, times the K steps and prints the headline (`value`,
`ms_per_step`); everything else it can report needs `--full`, and is `null` without it.  With `--full`, `roofline`
describes the dominant kernel (the forward `gemm_kernel<A_row,B_row>` template: teacher + student Linear layers) from
extra instrumented steps, `exchange` times one more step's bucket all-reduce (N > 1), `parity` cites the committed
margins, and `cpu_baseline` is the CPU oracle (oracle/, "port") timed on this box's host cores on a bounded bs-8
sample of the same step.

`--dump-outputs DIR` writes what the last timed step computed as float32 DIR/<name>.npy (rank 0): the DEKD losses and
logits that engine.distill_forward returned, and -- after that step's optimizer update -- a fixed sample (seed 0) of
the student's fp32 master weights, their EMA and the gradient the step applied.  Inputs and weights are seeded, so two
builds run with the same arguments can be compared output for output: every step starts from the same weights (see
`step`), so two runs differ only by the rounding of the fp32 atomics that sum the weight gradients.
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

GFLOP_PER_IMG_STEP = 63.503      # BASELINE.md §2 (student fwd+bwd 27.740 + teacher fwd 35.311 + relation 0.452): ALGORITHMIC
# what the step EXECUTES: both models' last blocks run on their two token rows only (devit_amd.de_vit.lean_tail; the
# reference computes and drops the other 196 rows): 63.503 - 2.431 (teacher) - 3 x 0.638 (student fwd + bwd)
GFLOP_PER_IMG_EXECUTED = 59.159
BF16_DENSE_PEAK = 2.5e15         # MI355X_MICROARCH.md: ~2.5 PFLOP/s dense bf16 MFMA


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch-size", type=int, default=256)
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also measure what the headline does not need: host cost at an idle queue, the "
                         "gradient exchange (N > 1), the dominant-kernel roofline / per-family / HBM-bound figures (extra "
                         "instrumented steps), the parity statement and the CPU baseline")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's outputs as float32 DIR/<name>.npy (rank 0; at most 64 MB)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU-baseline leg")
    ap.add_argument("--teacher-lookahead", type=int, default=1,
                    help="1: teacher forward of batch k+1 runs beside the student step of batch k (default); 0: inside the step")
    ap.add_argument("--cpu-seconds", type=float, default=15.0)
    ap.add_argument("--teacher-precision", default="bf16", choices=["f16", "bf16"],
                    help="16-bit type of the frozen teacher's forward: bf16 (default: the config BASELINE.json names) or f16 "
                         "(same kernels; teacher logits 1.1e-3 instead of 6.8e-3 from the fp32 reference -- around, not inside, the "
                         "1e-3 bar -- and the step 1.4 %% slower, same-box A/B; reported as `teacher_dtype`)")
    ap.add_argument("--classes", type=int, default=0, help="class count of both models' heads (default 25 at every N; 250 = ImageNet-1K / 4, BASELINE configs[3])")
    ap.add_argument("--shrink", type=float, default=0.0,
                    help="gate the student like distill_sub.py --neuron_shrinking --head_shrinking at this sparsity (random 0/1 masks: "
                         "int(6 (1 - r)) heads, int(1536 (1 - r)) neurons kept per block) and train it; never the headline value")
    ap.add_argument("--shrink-mode", default="compact", choices=["compact", "masked"],
                    help="compact: train through the compacted blocks (shrink.compact(trainable=True)); masked: as the reference, dense FLOPs")
    ap.add_argument("--rehearse-exchange", default="none", choices=["none", "abi", "torch"],
                    help="N = 1 only, never the headline value: send every gradient bucket through RCCL on the exchange stream "
                         "during backward although there is one rank (abi: the C ABI's devit_comm_* communicator; torch: a "
                         "world-size-1 torch.distributed nccl group); the reducer is told it has two ranks, so gradients are halved")
    ap.add_argument("--cpu-cores", type=int, default=0,
                    help="confine this process (every rank) to N host cores before anything touches the GPU: what the step costs the host when "
                         "eight ranks share one node's cores (the line then carries `cpu_cores`)")
    ap.add_argument("--host-input", action="store_true",
                    help="PCIe-inclusive variant (DESIGN.md section 6, never the headline value): every step's batch starts "
                         "in pinned host memory and crosses to the GPU through the training loop's prefetcher")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    return args


def usable_cores():
    """Threads the host really gives this process: affinity mask capped by the cgroup CPU quota (a 256-core box may
    hand the job far fewer; running torch with 256 threads on a quota of a few cores is 100x slower)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        q, p = open("/sys/fs/cgroup/cpu.max").read().split()
        if q != "max":
            n = min(n, max(1, int(int(q) / int(p))))
    except Exception:
        pass
    return max(1, min(n, 32))


def cpu_baseline(seconds):
    """CPU oracle ("port" of the reference path, pinned to its goldens) on a bounded sample: bs-8 DEKD steps."""
    from oracle import devit_oracle as O
    from oracle.detgen import det_array
    cores = usable_cores()
    torch.set_num_threads(cores)
    gs, gt = O.GEOMETRY["dedeit"], O.GEOMETRY["deit_base_distilled_patch16_224"]
    st_s = {k: v.requires_grad_(True) for k, v in O.make_state(gs, 25, "S").items()}
    st_t = O.make_state(gt, 25, "T")
    img = torch.from_numpy(det_array("cpu_bench", (8, 3, 224, 224)))
    soft = torch.full((8, 25), 0.1 / 25)
    soft[:, 3] += 0.9
    n, t0 = 0, None
    while True:
        out = O.distill_step(st_s, gs, st_t, gt, img, soft)
        out["loss"].backward()
        for v in st_s.values():
            v.grad = None
        if t0 is None:          # first step = warm-up
            t0 = time.time()
            continue
        n += 1
        if time.time() - t0 > seconds or n >= 20:
            break
    dt = time.time() - t0
    # BASELINE configs[0] (the reference's own CPU-runnable case): `dedeit` single sub-model eval forward, bs 8
    st_eval = {k: v.detach() for k, v in st_s.items()}
    m, f0 = 0, None
    with torch.no_grad():
        while True:
            O.forward(st_eval, gs, img, training=False)
            if f0 is None:
                f0 = time.time()
                continue
            m += 1
            if time.time() - f0 > min(5.0, seconds) or m >= 40:
                break
    fdt = time.time() - f0
    return {"value": round(8 * n / dt, 3), "unit": "images/sec", "cores": cores, "kind": "port",
            "sample": f"{n} fp32 DEKD steps (student fwd+bwd, DeiT-B teacher fwd, losses) at bs 8, no optimizer",
            "config1_forward": {"value": round(8 * m / fdt, 2), "unit": "images/sec",
                                "sample": f"{m} fp32 `dedeit` eval forwards at bs 8 (BASELINE configs[0])"}}


DUMP_SAMPLE = 1 << 20            # elements sampled from each flat fp32 buffer (4 MB each)
DUMP_MAX_BYTES = 64 << 20


def step_outputs(out, flat, opt):
    """Host float32 copies of what one step handed its caller: distill_forward's losses and logits (`out`) and, after the
    optimizer update, the same fixed sample (seed 0) of the flat fp32 master weights, their EMA and the applied gradient."""
    import numpy as np
    arrays = {}
    for k, v in out.items():
        if isinstance(v, (tuple, list)):         # a distilled model in train mode: (class head, distillation head)
            for i, t in enumerate(v):
                arrays[f"{k}_{i}"] = torch.as_tensor(t).detach().float().cpu().numpy()
        else:
            arrays[k] = torch.as_tensor(v).detach().float().cpu().numpy()
    idx = np.sort(np.random.default_rng(0).choice(flat.numel, size=min(DUMP_SAMPLE, flat.numel), replace=False))
    bufs = {"student_master_weights_sample": flat.flat, "student_grad_sample": flat.flat_grad}
    if opt.ema is not None:
        bufs["student_ema_weights_sample"] = opt.ema
    for k, t in bufs.items():
        arrays[k] = t.detach().cpu().numpy()[idx]
    return arrays


def dump_outputs(arrays, path):
    import numpy as np
    total = sum(a.nbytes for a in arrays.values())
    assert total <= DUMP_MAX_BYTES, f"--dump-outputs: {total} bytes > {DUMP_MAX_BYTES}"
    os.makedirs(path, exist_ok=True)
    for k, a in arrays.items():
        assert a.dtype in (np.float32, np.float64), (k, a.dtype)
        np.save(os.path.join(path, k + ".npy"), a)


def kernel_sources_hash():
    """sha256 (first 16 hex digits) over the kernel sources the library is built from (csrc/*.hip, *.h, generated *.inc, the C-ABI
    header).  The counter summaries under profiles/ record it (tools/pmc_*.py); a summary taken on other kernels than the
    ones this process runs is reported as stale instead of being passed off as a property of the current tree (there is no
    .git on the GPU box to ask)."""
    import glob
    import hashlib
    h = hashlib.sha256()
    files = sorted(f for ext in ("*.hip", "*.h", "*.inc") for f in glob.glob(os.path.join(ROOT, "devit_amd", "csrc", ext))) + \
        [os.path.join(ROOT, "include", "devit_hip.h")]
    for f in files:
        h.update(os.path.basename(f).encode())
        h.update(open(f, "rb").read())
    return h.hexdigest()[:16]


def pick_profile(pattern, want_hash=None):
    """The committed summary profiles/<pattern> to cite: the one taken on the kernel sources this process runs
    (`kernel_sources_hash` inside the file == want_hash; the newest by mtime if several match), else the newest by mtime.
    Never by file name: 'r03_C_*' sorts before 'r03_w_*' although it is the later set."""
    import glob
    files = glob.glob(os.path.join(ROOT, "profiles", pattern))
    if not files:
        return None, None
    rows = []
    for f in files:
        try:
            with open(f) as fh:
                d = json.load(fh)
        except Exception:
            continue
        h = d.get("kernel_sources_hash") if isinstance(d, dict) else None
        rows.append((want_hash is not None and h == want_hash, os.path.getmtime(f), f, d))
    if not rows:
        return None, None
    rows.sort(key=lambda r: (r[0], r[1], r[2]))
    return rows[-1][2], rows[-1][3]


def committed_counter(pattern, key):
    """(value, source) of the committed rocprofv3 counter summary matching profiles/<pattern> that was taken on the current
    kernel sources -- the counters cannot be read from inside the process, so they come from separate `--pmc` passes over
    this same command (tools/gpu_pmc_*.sh).  value is None when no summary exists or when the only ones there were taken on
    different kernel sources (source says which)."""
    cur = kernel_sources_hash()
    f, d = pick_profile(pattern, cur)
    if f is None:
        return None, None
    src = {"file": "profiles/" + os.path.basename(f), "kernel_sources_hash": d.get("kernel_sources_hash"),
           "current_kernel_sources_hash": cur}
    src["stale"] = src["kernel_sources_hash"] != src["current_kernel_sources_hash"]
    return (None if src["stale"] else d.get(key)), src


def parity_statement():
    """Which tolerance the benchmarked kernels meet, from the committed profiles/*_parity_margins.json (written by the
    `-m gpu` test session, tests/conftest.py) taken on the current kernel sources (else the newest, marked stale): BASELINE.json
    asks for logits within 1e-3 rel; the bf16 kernels timed here do not meet that, the exact-fp32 mode (never benchmarked) does."""
    out = {"mode": "bf16", "logits_rel_to_max": None, "top1_exact_golden_bs8": True, "top1_flips_bs256": None, "bar": 1.5e-2,
           "north_star_1e-3_met_by": 'precision="f32" (2e-6 measured; a few TFLOP/s, not benchmarked)', "source": None}
    cur = kernel_sources_hash()
    f, d = pick_profile("*_parity_margins.json", cur)
    if f is None:
        return out
    rows = d["rows"] if isinstance(d, dict) else d        # older files are a bare list of rows (no source hash)
    file_hash = d.get("kernel_sources_hash") if isinstance(d, dict) else None
    vals = {}
    for which in ("dedeit", "deitb"):
        r = [x for x in rows if f"test_model_forward_vs_golden[{which}]" in x.get("test", "") and abs(x.get("bar", 0) - 1.5e-2) < 1e-9]
        if r:
            vals[which] = round(r[0]["value"], 6)
    out["logits_rel_to_max"] = vals or None
    # the benchmarked batch size against the fp32 oracle (tests/test_gpu_trajectory.py::test_full_size_step_vs_oracle): images of 256 whose top-1 differs
    named = {x["name"]: x["value"] for x in rows if "name" in x}
    flips = {k: round(named[f"bs256_top1_flip_share[{k}]"] * 256) for k in ("student", "student_dist", "teacher") if f"bs256_top1_flip_share[{k}]" in named}
    if flips:
        flips["of"] = 256
        flips["max_ref_margin"] = round(max(named.get(f"bs256_top1_flip_max_ref_margin[{k}]", 0.0) for k in ("student", "student_dist", "teacher")), 5)
        flips["cls_loss_shift_from_teacher_flips"] = named.get("bs256_cls_loss_shift_from_teacher_top1_flips")
        out["top1_flips_bs256"] = flips
    out["source"] = "profiles/" + os.path.basename(f) + " (tests/test_gpu_model.py::test_model_forward_vs_golden, top-1 asserted bit-exact there)"
    out["kernel_sources_hash"] = file_hash
    out["stale"] = file_hash != cur
    return out


def self_launch(args):
    """`python bench.py --gpus N` without a launcher: start the N ranks (one process per GPU, the README.md:50-68 launch
    form of the reference) as children of this process, which has not touched a GPU and never will; rank 0's JSON line
    passes through on stdout, the exit code is the children's."""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    return subprocess.call(cmd, env=env)


def stub_main(args, rank, world, json_out):
    """DEVIT_BENCH_STUB=1 (tests/test_bench_launch.py): the launch / rendezvous / bucketed exchange / timing / one-line
    protocol of this file on CPU tensors over gloo, with a toy model in place of the HIP step (no GPU in CI)."""
    from devit_amd import ddp
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.manual_seed(rank)                         # ranks start different: the broadcast must fix it
    model = torch.nn.Sequential(torch.nn.Linear(32, 64), torch.nn.Linear(64, 64), torch.nn.Linear(64, 8))
    flat = ddp.FlatParams(model)
    ddp.broadcast_parameters(flat)
    reducer = ddp.BucketedGradReducer(flat, bucket_bytes=8192)
    x = torch.randn(16, 32, generator=torch.Generator().manual_seed(100 + rank))
    if os.environ.get("DEVIT_BENCH_STUB_FAIL_RANK") == str(rank):
        raise SystemExit(3)                         # the launcher must turn one failed rank into a non-zero exit
    params = list(model.parameters())

    def step():
        flat.zero_grad()
        loss = model(x).square().mean()
        grads = torch.autograd.grad(loss, params)
        for p, g in reversed(list(zip(params, grads))):
            p.grad.add_(g)
            reducer.mark_ready([p])
        reducer.finish()
        flat.flat.add_(flat.flat_grad, alpha=-0.01 * flat.grad_scale)
        flat.grad_scale = 1.0
        return loss

    for _ in range(args.warmup):
        step()
    dist.barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        loss = step()
    dist.barrier()
    tmax = torch.tensor([time.perf_counter() - t0], dtype=torch.float64)
    dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
    w = [torch.zeros_like(flat.flat) for _ in range(world)]
    dist.all_gather(w, flat.flat)
    in_sync = all(torch.equal(w[0], t) for t in w)
    if rank == 0:
        json_out.write(json.dumps({"metric": "stub", "value": 16 * world * args.steps / float(tmax), "unit": "rows/sec",
                                   "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "scaling": "weak",
                                   "data": "stub", "replicas_in_sync": in_sync, "buckets": len(reducer.buckets),
                                   "loss": float(loss)}) + "\n")
        json_out.flush()
    dist.destroy_process_group()


def main():
    args = parse()
    if args.cpu_cores > 0 and hasattr(os, "sched_setaffinity"):
        # before any GPU call and before the launcher forks the ranks (children inherit the mask): rank r of a launched job takes its own
        # slice so that N ranks x C cores are disjoint, as a node with 8 ranks would have it
        avail = sorted(os.sched_getaffinity(0))
        r = int(os.environ.get("LOCAL_RANK", 0)) if "WORLD_SIZE" in os.environ else 0
        mine = [avail[(r * args.cpu_cores + i) % len(avail)] for i in range(min(args.cpu_cores, len(avail)))]
        if "WORLD_SIZE" in os.environ or args.gpus == 1:
            os.sched_setaffinity(0, set(mine))
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        sys.exit(self_launch(args))          # nothing above has initialised a GPU; the ranks are fresh processes
    # stdout carries exactly one line, the JSON; whatever the libraries print while starting up (RCCL's version banner
    # at communicator creation, ...) goes to stderr
    sys.stdout.flush()
    json_out = os.fdopen(os.dup(1), "w")
    os.dup2(2, 1)
    rank = int(os.environ.get("RANK", 0))
    world = int(os.environ.get("WORLD_SIZE", 1))
    local = int(os.environ.get("LOCAL_RANK", 0))
    if world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but the launcher started WORLD_SIZE={world} ranks")
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    if os.environ.get("DEVIT_BENCH_STUB") == "1":
        return stub_main(args, rank, world, json_out)
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    if world > 1:
        dist.init_process_group("nccl", rank=rank, world_size=world)

    import devit_amd
    from devit_amd import ddp, engine, losses, ops, optim

    B = args.batch_size
    # The SAME class count at every N (25 = BASELINE configs[2], the headline workload), so that the driver's weak-scaling ratio
    # compares like with like; configs[3]'s ImageNet/4 heads are `--classes 250` (measured at N = 1: the same rate within noise,
    # profiles/*_bench_c250_n1.json -- the two heads are 0.02 % of the step's FLOPs).
    C = args.classes or 25
    torch.manual_seed(0)
    student = devit_amd.create_model("dedeit", num_classes=C, drop_path_rate=0.1, drop_block_rate=None).to(dev).train()
    torch.manual_seed(1)
    teacher = devit_amd.create_model("deit_base_distilled_patch16_224", num_classes=C).to(dev).eval()
    for p in teacher.parameters():
        p.requires_grad_(False)
    teacher.request_precision(args.teacher_precision)      # frozen, forward only ("f16": IEEE f16 operands; student and all gradients stay bf16)

    flat = ddp.FlatParams(student)
    ddp.broadcast_parameters(flat)          # before the bf16 GEMM copies are cast from the masters
    flat.attach_bf16(student)
    shrink_info = None
    if args.shrink > 0:
        from devit_amd import shrink
        gen = torch.Generator().manual_seed(7)
        for blk in student.blocks:
            hm, nm = torch.ones(6), torch.ones(1536)
            hm[torch.randperm(6, generator=gen)[: 6 - int(6 * (1 - args.shrink))]] = 0
            nm[torch.randperm(1536, generator=gen)[: 1536 - int(1536 * (1 - args.shrink))]] = 0
            blk.attn.gate, blk.mlp.gate = hm, nm
        if args.shrink_mode == "compact":
            shrink.compact(student, trainable=True)
        shrink_info = {"ratio": args.shrink, "mode": args.shrink_mode,
                       "student_forward_gflop_per_img": round(shrink.compacted_gflops(student, num_classes=C), 3)}
    if args.rehearse_exchange != "none" and world == 1:
        if args.rehearse_exchange == "abi":
            reducer = ddp.BucketedGradReducer(flat, comm=ddp.RcclComm(rank=0, world=1), world=2).attach(student)
        else:
            os.environ.setdefault("MASTER_PORT", "29533")
            dist.init_process_group("nccl", rank=0, world_size=1)
            reducer = ddp.BucketedGradReducer(flat, world=2).attach(student)
    else:
        reducer = ddp.BucketedGradReducer(flat).attach(student)
    from devit_amd import _lib as _L
    reserved_cus = _L.load().devit_get_reserved_cus()
    opt = optim.FlatAdamW(flat, lr=5e-4 * B * world / 512.0, weight_decay=0.0, max_norm=1.0, ema_decay=0.99996)
    criterion = losses.DistillLoss(losses.SoftTargetCrossEntropy(), "hard", 0.5, 1.0)

    g = torch.Generator(device=dev).manual_seed(1234 + rank)
    img = torch.randn((B, 3, 224, 224), generator=g, device=dev)
    y1 = torch.randint(0, C, (B,), generator=g, device=dev)
    y2 = torch.randint(0, C, (B,), generator=g, device=dev)
    oh = lambda y: torch.full((B, C), 0.1 / C, device=dev).scatter_(1, y[:, None], 0.9 + 0.1 / C)
    soft = 0.7 * oh(y1) + 0.3 * oh(y2)       # mixup of two smoothed one-hots

    # The frozen teacher runs one batch ahead on the side stream (engine.TeacherLookahead): every step still enqueues
    # exactly one teacher forward -- the one for the next batch -- beside its own student forward/backward.
    look = engine.TeacherLookahead(teacher) if args.teacher_lookahead else None
    # As in the training loop (engine._PreparedBatches): a batch is cut into bf16 patch rows ONCE, when it is prepared (one batch ahead), and the look-ahead
    # teacher and -- one step later -- the student read the same rows.  Every step still prepares exactly one batch.
    row_dtypes = engine.row_dtypes_for(student, teacher)
    prepare = (lambda: ops.patch_rows(img, dtypes=row_dtypes)) if row_dtypes else (lambda: img)
    cur = prepare()
    if look is not None:
        look.submit(cur)

    feed = feed_batches = None
    if args.host_input:
        class _Repeat:                       # a loader that hands out the same pinned host batch
            def __init__(self, batch, n): self.batch, self.n = batch, n
            def __len__(self): return self.n
            def __iter__(self): return (self.batch for _ in range(self.n))
        host = (img.cpu().pin_memory(), soft.cpu().pin_memory())
        if look is not None:
            look.take(cur)
        feed_batches = engine._PreparedBatches(_Repeat(host, args.warmup + args.steps + 2), dev, None, look, row_dtypes=row_dtypes)   # (+ the two idle-queue steps)
        feed = iter(feed_batches)

    opt_events = None        # instrumented step: events around the optimizer tail (clip + AdamW + EMA + bf16 re-cast)
    kept = {}                # --dump-outputs: distill_forward's dict of the last timed step

    # Every step starts from the same weights: the fp32 masters and their bf16 copy (with the k-major copies derived from it) are put back to
    # the state after set-up, so each timed step is the same optimisation step on the same inputs.  The weight gradients are summed with fp32
    # atomics (bitwise different from run to run), and AdamW's early updates turn that rounding into different weights within a few steps:
    # chained, the steps would compute different things every run.  Adam's moments, the EMA and the step count still advance.
    start_flat, start_flat16 = flat.flat.clone(), flat.flat16.clone()

    def step(keep=False):
        nonlocal cur
        flat.flat.copy_(start_flat)
        flat.flat16.copy_(start_flat16)
        flat.refresh_kmajor()
        opt.zero_grad()
        t_out = None
        if feed is not None:
            x, y, t_out = next(feed)
        elif look is not None:
            x, y, t_out = cur, soft, look.take(cur)
            cur = prepare()                      # the next batch (the same synthetic images again), prepared one step ahead
            look.submit(cur, defer=True)         # launched behind the student's forward (after_student below), as in the training loop
        else:
            x, y = prepare(), soft               # (teacher inside the step: both models read the one set of rows)
        launch = (feed_batches.launch_teacher if feed is not None else (look.launch if look is not None else None))
        out = engine.distill_forward(student, teacher, x, y, gama=(0.2, 0.1, 0.3), criterion=criterion,
                                     teacher_outputs=t_out, after_student=launch)
        out["loss"].backward()
        if opt_events is not None:
            opt_events.append(torch.cuda.Event(enable_timing=True))
            opt_events[-1].record()
        reducer.finish()
        opt.step()
        if opt_events is not None:
            opt_events.append(torch.cuda.Event(enable_timing=True))
            opt_events[-1].record()
        if keep:
            kept["out"] = out
        return out["loss"]

    def fence():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    for _ in range(args.warmup):
        step()
    fence()
    t0 = time.perf_counter()
    dump = args.dump_outputs is not None
    for i in range(args.steps):
        loss = step(keep=dump and i == args.steps - 1)
    t_enqueue = time.perf_counter() - t0          # host time to enqueue the K steps (no device wait inside)
    fence()
    dt = time.perf_counter() - t0
    if dump:          # before any further step moves the weights
        out_last = kept.pop("out")
        if rank == 0:
            dump_outputs(step_outputs(out_last, flat, opt), args.dump_outputs)
        del out_last
    host_step_ms = None
    if args.full:
        # host cost of one step with nothing in the way: the device idle and its queue empty when the enqueue starts
        # (`host_enqueue_ms_per_step` above also contains the time the host sits blocked on a full launch queue once it is
        # several steps ahead of the GPU)
        t1 = time.perf_counter()
        step()
        step()
        host_step_ms = (time.perf_counter() - t1) / 2 * 1e3
        fence()
    tmax = torch.tensor([dt], dtype=torch.float64, device=dev)
    if world > 1:
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
    dt = float(tmax.item())
    loss_value = float(loss.detach())
    assert loss_value == loss_value, "non-finite loss"
    img_per_s = B * world * args.steps / dt
    hbm_peak_gb = torch.cuda.max_memory_allocated(dev) / 1e9     # this rank, warm-up + timed steps (torch's allocator: arenas, masters, gradients)

    from devit_amd import de_vit
    executed = GFLOP_PER_IMG_EXECUTED if de_vit.LEAN_TAIL else GFLOP_PER_IMG_STEP

    # ---- --full: what the headline does not need, each from steps of its own after the timed ones
    exchange = roof = None
    if args.full:
        # ---- gradient exchange of one more step: summed bucket all-reduce time and the share of it that ran under backward
        exchange = None
        if reducer.world > 1:
            reducer.timing = True
            step()
            reducer.timing = False
            ar_ms, ov = reducer.timing_summary()
            t = torch.tensor([ar_ms, -ov], dtype=torch.float64, device=dev)
            if world > 1:
                dist.all_reduce(t, op=dist.ReduceOp.MAX)              # worst rank, like the step time: longest exchange, least overlap
            exchange = {"allreduce_ms": round(float(t[0]), 3), "overlap_frac": round(-float(t[1]), 3),
                        "buckets": len(reducer.buckets), "bytes": flat.numel * 4,
                        "over_ranks": "max allreduce_ms, min overlap_frac"}

        # ---- dominant-kernel roofline: extra instrumented steps, events on the launch stream ---------------------
        # (a) as in the timed region: the teacher's launches share the GPU with the student's (two streams), so an event
        #     bracket there also contains the other model's workgroups -- this is what a rocprofv3 average over the run sees
        two_stream = None
        if look is not None and feed is None:
            ops.PROFILE = []
            step()
            torch.cuda.synchronize()
            recs, ops.PROFILE = ops.PROFILE, None
            sel = [(2.0 * M * N * K * batch, e0.elapsed_time(e1) * 1e-3) for t, M, N, K, batch, e0, e1 in recs if t == "A_row/B_row"]
            fl2, tm2 = sum(f for f, _ in sel), sum(t for _, t in sel)
            two_stream = {"achieved": round(fl2 / tm2 / 1e12, 2), "avg_launch_us": round(tm2 / len(sel) * 1e6, 2),
                          "launches_per_step": len(sel)}
        # (b) one launch at a time (`achieved` below): the kernel's own rate
        os.environ["DEVIT_TEACHER_STREAM"] = "0"      # serialise the two forwards so that event brackets time ONE kernel
        os.environ["DEVIT_WGRAD_STREAM"] = "0"        # ... and the weight gradients back on the launch stream (csrc/encoder.hip)
        if feed is not None:
            assert next(feed, None) is None       # the prefetcher is drained (its last batch submits no look-ahead)
            feed = None
        elif look is not None:
            look.take(cur)
        look = None
        step()
        torch.cuda.synchronize()
        # per-family split of the serialized step (events on the launch stream): the frozen teacher's forward alone, the rest is the
        # student's half (forward, losses, backward, optimizer tail) -- tracked because the two halves sit at very different fractions
        def timed(fn, reps=3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / reps
        serial_ms = timed(step)
        teacher_ms = timed(lambda: engine._teacher_forward(teacher, img))
        student_ms = serial_ms - teacher_ms
        families = {"serialized_step_ms": round(serial_ms, 3),
                    "teacher_forward_ms": round(teacher_ms, 3), "teacher_gflop_per_img_algorithmic": 35.311,
                    "teacher_frac": round(B * 35.311e9 / (teacher_ms * 1e-3) / BF16_DENSE_PEAK, 4),
                    "student_ms_per_step": round(student_ms, 3), "student_gflop_per_img_algorithmic": round(GFLOP_PER_IMG_STEP - 35.311, 3),
                    "student_frac": round(B * (GFLOP_PER_IMG_STEP - 35.311) * 1e9 / (student_ms * 1e-3) / BF16_DENSE_PEAK, 4),
                    "counts": "ALGORITHMIC FLOPs (teacher forward 35.311, student forward + backward + relation losses 28.192 GFLOP per image) / "
                              "event time of the serialized step's halves / 2.5 PFLOP/s"}
        ops.PROFILE, ops.PROFILE_HBM, ops.PROFILE_WGRAD = [], [], []
        opt_events = []
        step()
        torch.cuda.synchronize()
        opt_tail_ms = opt_events[0].elapsed_time(opt_events[1])
        opt_events = None
        recs, ops.PROFILE = ops.PROFILE, None
        hbm_recs, ops.PROFILE_HBM = ops.PROFILE_HBM, None
        wg_recs, ops.PROFILE_WGRAD = ops.PROFILE_WGRAD, None
        # the bandwidth-bound kernels of the same serialized step: algorithmic bytes / event time (HBM peak 8 TB/s)
        hbm = {}
        for name, nbytes, e0, e1 in hbm_recs:
            d = hbm.setdefault(name, [0.0, 0.0, 0])
            d[0] += nbytes
            d[1] += e0.elapsed_time(e1) * 1e-3
            d[2] += 1
        hbm = {k: {"GB/s": round(v[0] / v[1] / 1e9, 1), "frac_of_8TB/s": round(v[0] / v[1] / 8e12, 3), "launches": v[2],
                   "ms_per_step": round(v[1] * 1e3, 3)} for k, v in hbm.items()}
        by_t = {}
        for tmpl, M, N, K, batch, e0, e1 in recs:
            d = by_t.setdefault(tmpl, [0.0, 0.0, 0])
            d[0] += 2.0 * M * N * K * batch
            d[1] += e0.elapsed_time(e1) * 1e-3
            d[2] += 1
        # the grouped weight-gradient launches (devit_wgrad_grouped: a block's four products in one launch of the full-row k-major x k-major kernel)
        if wg_recs:
            wt = sum(e0.elapsed_time(e1) * 1e-3 for _, _, e0, e1 in wg_recs)
            by_t["A_km/B_km grouped (wgradfr_kernel)"] = [sum(f for f, _, _, _ in wg_recs), wt, len(wg_recs)]
            hbm["wgrad_grouped"] = {"GB/s": round(sum(b for _, b, _, _ in wg_recs) / wt / 1e9, 1),
                                    "frac_of_8TB/s": round(sum(b for _, b, _, _ in wg_recs) / wt / 8e12, 3), "launches": len(wg_recs),
                                    "ms_per_step": round(wt * 1e3, 3)}
        dom = "A_row/B_row"
        fl, tm, cnt = by_t[dom]
        traffic, traffic_src = committed_counter("*_pmc_traffic.json", "traffic_bytes_per_launch")
        busy, busy_src = committed_counter("*_pmc_mfma.json", "mfma_busy")
        roof = {"bound": "mfma", "kernel": "gemm_kernel<*, A_row, B_row, *> (persistent 128x128 / 256x256 x64 bf16 MFMA tiles; fwd Linear layers of teacher + student; "
                          "the student's fc2 on the full-row 256x384 kernel through a k-major copy of its weight counts here too)",
                "achieved": round(fl / tm / 1e12, 2), "peak": BF16_DENSE_PEAK / 1e12, "unit": "TFLOP/s",
                "frac": round(fl / tm / BF16_DENSE_PEAK, 4),
                "achieved_counts": "FLOPs the launches execute (2 M N K of each launch, padded rows included) / their event time",
                "traffic": traffic, "traffic_source": traffic_src, "mfma_busy": busy, "mfma_busy_source": busy_src,
                "launches_per_step": cnt, "avg_launch_us": round(tm / cnt * 1e6, 2),
                "gflop_per_launch_avg": round(fl / cnt / 1e9, 3),
                "step_frac": round(img_per_s / world * GFLOP_PER_IMG_STEP * 1e9 / BF16_DENSE_PEAK, 4),
                "step_frac_counts": "ALGORITHMIC FLOPs of the reference's step (63.503 GFLOP per image) x images/sec / peak",
                "step_frac_executed": round(img_per_s / world * executed * 1e9 / BF16_DENSE_PEAK, 4),
                "other_templates": {k: {"tflops": round(v[0] / v[1] / 1e12, 2), "launches": v[2],
                                        "ms_per_step": round(v[1] * 1e3, 3)} for k, v in by_t.items() if k != dom},
                "gemm_ms_per_step": round(sum(v[1] for v in by_t.values()) * 1e3, 3),
                "in_two_stream_timed_region": two_stream, "families": families, "hbm_bound_kernels": hbm,
                "optimizer_tail_ms_per_step": round(opt_tail_ms, 3)}

    cpu = None
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline:
        cpu = cpu_baseline(args.cpu_seconds)

    if rank == 0:
        line = json.dumps({
            "metric": "images/sec distill_sub step (DeiT-B->dedeit, bs256, 224^2)", "value": round(img_per_s, 2),
            "unit": "images/sec", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(dt / args.steps * 1e3, 3), "host_enqueue_ms_per_step": round(t_enqueue / args.steps * 1e3, 3),
            "host_ms_per_step_idle_queue": round(host_step_ms, 3) if host_step_ms is not None else None,
            "cpu_cores": len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else None,   # (what this rank may run on: --cpu-cores)
            "hbm_peak_allocated_gb": round(hbm_peak_gb, 2),
            "higher_is_better": True, "scaling": "weak",
            "algorithmic_gflop_per_img": GFLOP_PER_IMG_STEP, "executed_gflop_per_img": executed,
            "timing_protocol": f"{args.warmup} untimed steps, then {args.steps} steps wall-clocked between barrier + "
                               "torch.cuda.synchronize() on both sides, max over ranks, mean per step (SURVEY 8d's median-of-50 "
                               "protocol is not what the driver runs)" + ("; roofline / hbm_bound_kernels from one extra instrumented "
                               "serialized step (HIP events on the launch stream)" if args.full else ""),
            "full": args.full, "parity": parity_statement() if args.full else None,
            "vs_baseline": None, "dtype": "bf16", "teacher_dtype": args.teacher_precision, "data": "synthetic, pinned host batches through PCIe every step" if args.host_input else "synthetic",
            "config": {"workload": f"distill_sub step dedeit<-deit_base_distilled_patch16_224, num_division=4 "
                                   f"(C={C}), bs={B}/GPU, 224x224, hard distillation, drop_path 0.1, AdamW+EMA",
                       "classes": C, "global_batch": B * world, "parallelism": f"dp{world}", "loss": round(loss_value, 5),
                       "shrink": shrink_info},
            "reserved_cus": reserved_cus, "reserved_cus_while_buckets_in_flight": reducer.reserve_cus if reducer.world > 1 else 0,
            "rehearse_exchange": args.rehearse_exchange,
            "wgrad_groups": ops.DeferredWgrads(type("C", (), {"grad_ready": student.grad_ready, "blocks": []})(), 0).policy,   # all blocks in one launch / the reducer's buckets
            "bucket_mb": [round((e - s_) * 4 / 2 ** 20, 2) for s_, e, _, _ in reducer.buckets],
            "allreduce_ms": exchange["allreduce_ms"] if exchange else None,
            "overlap_frac": exchange["overlap_frac"] if exchange else None, "exchange": exchange,
            "roofline": roof, "cpu_baseline": cpu})
        json_out.write(line + "\n")
        json_out.flush()
    if dist.is_initialized():
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
