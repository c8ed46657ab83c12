"""Optimizer tail of the DEKD step on flat buffers: global-norm clip + update + EMA + bf16 weight re-cast in two launches (devit_sumsq_f32,
then the tail's step).  Replaces timm NativeScaler -> clip_grad_norm_ -> optimizer.step and ModelEma.update (engine.py:127,131-132; ~600 tiny
kernels in the reference).

Five tails on one frame (_FlatTail: the buffers, the scalar ring, the step's begin and end, the state dict), one for every optimizer the
reference's `--opt` reaches through timm's create_optimizer: FlatAdamW (`adamw`), FlatSGD (`momentum`, `nesterov`), FlatAdam (`adam`: L2 decay
coupled into the gradient) and FlatLamb (`lamb`, `lambc`: per-tensor trust ratios over a chunk table, three launches).  A class adds its
hyper-parameters and its one C call; create_flat_optimizer maps the command line to one of them."""
import math
import re

import torch

from . import _lib as L
from ._lib import call, ptr, stream_ptr

OPT_NAMES = ("adamw", "adam", "momentum", "nesterov", "lamb", "lambc")


def no_decay_names(model):
    """Parameters timm's create_optimizer (distill_sub.py:340) puts into its weight_decay = 0 group whenever
    weight_decay > 0: 1-D tensors, `.bias`, and the names in model.no_weight_decay()."""
    skip = set(model.no_weight_decay()) if hasattr(model, "no_weight_decay") else set()
    return {n for n, p in model.named_parameters()
            if p.requires_grad and (p.ndim <= 1 or n.endswith(".bias") or n in skip)}


_STEM_NAMES = ("cls_token", "dist_token", "pos_embed")
LR_TABLE = 256          # entries of the kernels' lr_scales table: one for every value of a byte (include/devit_hip.h)


def layer_ids(names, depth):
    """{name: layer id} of layer-wise lr decay over a ViT of `depth` blocks (`--layer-decay`): cls_token, dist_token,
    pos_embed and patch_embed.* 0, blocks.<i>.* i + 1, everything else (norm, head, head_dist, resize_*) depth + 1.  A prefix in front of the
    name (`backbones.<k>.` of MultiViT, `module.`) changes nothing: blocks.<i>. is matched at any dot, the bare names at the path's end."""
    ids = {}
    for name in names:
        m = re.search(r"(^|\.)blocks\.(\d+)\.", name)
        if m:
            i = int(m.group(2))
            if i >= depth:
                raise ValueError(f"{name}: block {i} of a model of depth {depth}")
            ids[name] = i + 1
        elif name.split(".")[-1] in _STEM_NAMES or re.search(r"(^|\.)patch_embed\.", name):
            ids[name] = 0
        else:
            ids[name] = depth + 1
    return ids


def layer_decay_scales(names, depth, decay):
    """{name: scale}: scale(id) = decay^(depth + 1 - id), formed in float64 and rounded to fp32 -- the head and the final norm train at the
    scheduled lr, the last block at decay times it, the stem at decay^(depth + 1) times it"""
    return {n: float(torch.tensor(float(decay) ** (depth + 1 - i), dtype=torch.float64).to(torch.float32)) for n, i in layer_ids(names, depth).items()}


def model_depth(model):
    """len(model.blocks), or the common depth of a MultiViT's backbones"""
    if hasattr(model, "blocks"):
        return len(model.blocks)
    depths = {len(b.blocks) for b in getattr(model, "backbones", []) if hasattr(b, "blocks")}
    if len(depths) != 1:
        raise ValueError(f"--layer-decay: {type(model).__name__} has no blocks, or backbones of different depths {sorted(depths)}")
    return depths.pop()


def lr_scale_table(names, sizes, offsets, numel, lr_scales):
    """{name: scale} over a flat buffer -> (group bytes [numel / 4] uint8, table [256] fp32), both on the CPU: what the *_lrs entry points read.
    The distinct scales, as fp32, are numbered in ascending order behind group 0, which is scale 1: padding between tensors and tensors the dict
    does not name are in it, and so is every table entry no group uses.  Every granule of a tensor, its last partial one too, carries the
    tensor's group.  ValueError: a name the buffer does not hold, a negative or non-finite scale, more than 256 distinct scales."""
    unknown = sorted(set(lr_scales) - set(names))
    if unknown:
        raise ValueError(f"lr_scales: {unknown[0]} is not a tensor of the flat buffer")
    f32 = {}
    for n, s in lr_scales.items():
        s = float(s)
        if not math.isfinite(s) or s < 0:
            raise ValueError(f"lr_scales: {n} has scale {s}; a scale is finite and >= 0")
        f32[n] = float(torch.tensor(s, dtype=torch.float32))
    values = [1.0] + sorted(set(f32.values()) - {1.0})
    if len(values) > LR_TABLE:
        raise ValueError(f"lr_scales: {len(values)} distinct scales (1.0 included); the table has {LR_TABLE} entries")
    group_of = {v: g for g, v in enumerate(values)}
    table = torch.ones(LR_TABLE, dtype=torch.float32)
    table[:len(values)] = torch.tensor(values, dtype=torch.float32)
    group4 = torch.zeros(numel // 4, dtype=torch.uint8)
    for name, size, o in zip(names, sizes, offsets):
        if name in f32:
            group4[o // 4:(o + size + 3) // 4] = group_of[f32[name]]
    return group4, table


class _FlatTail:
    """What every optimizer over ddp.FlatParams shares: the buffers and the scalar ring (_setup), the surface the training loops use
    (param_groups[0]["lr"], zero_grad, max_norm, ema_state_dict), the step's frame and the state dict."""
    opt_name = "adamw"
    state_keys = ("m", "v")
    layer_decay = None      # what --layer-decay gave when the scales came from it (create_flat_optimizer): kept in the state dict

    def _setup(self, flat, lr, weight_decay, max_norm, ema_decay, no_decay, dyn_len, lr_scales=None):
        self.flat, self.weight_decay, self.max_norm, self.ema_decay = flat, weight_decay, max_norm, ema_decay
        dev = flat.flat.device
        self.no_decay4 = None
        if weight_decay and no_decay:
            mask = torch.zeros(flat.numel // 4, dtype=torch.uint8)
            for name, p, o in zip(flat.names, flat.params, flat.offsets):
                if name in no_decay:
                    mask[o // 4:(o + p.numel() + 3) // 4] = 1
            self.no_decay4 = mask.to(dev)
        # a learning rate per tensor, {name: scale}: one byte per granule into a table of 256 scales, and the step calls the *_lrs entry point
        self.lr_group4 = self.lr_scales = None
        if lr_scales is not None:
            group4, table = lr_scale_table(flat.names, [p.numel() for p in flat.params], flat.offsets, flat.numel, lr_scales)
            self.lr_group4, self.lr_scales = group4.to(dev), table.to(dev)
        for k in self.state_keys:
            setattr(self, k, torch.zeros_like(flat.flat))
        self.ema = flat.flat.clone() if ema_decay is not None else None
        self.step_count = 0
        self.param_groups = [{"lr": lr, "params": flat.params}]
        self.gnorm_sq = torch.zeros(1, dtype=torch.float32, device=dev)
        # per-step scalars (lr, bias corrections) travel through pinned memory with an async copy; the host runs ahead of
        # the GPU, so every step in flight needs its own slot (a ring far deeper than the launch queue)
        host = torch.zeros((256, dyn_len), dtype=torch.float32)
        self._dyn_host = host.pin_memory() if dev.type == "cuda" else host
        self._dyn = torch.zeros(dyn_len, dtype=torch.float32, device=dev)
        self._ws = torch.empty(4096, dtype=torch.uint8, device=dev)

    def _scalars(self, t):
        """the Adam family's `dyn` at step t: lr and the two bias corrections"""
        return self.param_groups[0]["lr"], 1.0 - self.betas[0] ** t, 1.0 - self.betas[1] ** t

    def _begin_step(self, scalars, need_norm=False):
        """step_count, the step's scalars into the device `dyn`, the gradient's squared norm when the step clips (or needs it) -> clip?"""
        L.require_device(self.flat.flat)
        self.step_count += 1
        slot = self._dyn_host[self.step_count % self._dyn_host.shape[0]]
        for i, s in enumerate(scalars(self.step_count)):
            slot[i] = s
        self._dyn.copy_(slot, non_blocking=True)
        f = self.flat
        clip = self.max_norm is not None and self.max_norm > 0
        if clip or need_norm:
            call("devit_sumsq_f32", ptr(f.flat_grad), f.numel, ptr(self.gnorm_sq), ptr(self._ws), self._ws.numel(),
                 stream_ptr())
        return clip

    def _end_step(self):
        self.flat.grad_scale = 1.0
        self.flat.refresh_kmajor()      # the kernel rewrote flat16 in place: the k-major weight copies derived from it follow

    def zero_grad(self, set_to_none=False):
        self.flat.zero_grad()

    def ema_state_dict(self, model):
        """EMA weights keyed like model.state_dict() (timm get_state_dict(model_ema), distill_sub.py:429)."""
        if self.ema is None:
            return None
        f, out = self.flat, {}
        by_id = {id(p): n for n, p in model.named_parameters()}
        for p, o in zip(f.params, f.offsets):
            out[by_id[id(p)]] = self.ema[o:o + p.numel()].view_as(p).clone()
        return {k: out[k] for k in model.state_dict() if k in out}

    def _check_kind(self, sd):
        kind = sd.get("opt", "adamw")           # FlatAdamW's checkpoints carry no name
        if kind != self.opt_name:
            raise ValueError(f"optimizer state of --opt {kind} cannot be loaded into --opt {self.opt_name}")

    def state_dict(self):
        sd = {"opt": self.opt_name, "ema": self.ema, "step": self.step_count, "lr": self.param_groups[0]["lr"]}
        sd.update({k: getattr(self, k) for k in self.state_keys})
        if self.layer_decay is not None:        # the flag, not the scales: they are rebuilt from it
            sd["layer_decay"] = self.layer_decay
        return sd

    def load_state_dict(self, sd):
        self._check_kind(sd)
        if sd.get("layer_decay") != self.layer_decay:
            raise ValueError(f"optimizer state of --layer-decay {sd.get('layer_decay')} cannot be loaded into --layer-decay {self.layer_decay}")
        for k in self.state_keys:
            getattr(self, k).copy_(sd[k])
        if self.ema is not None and sd.get("ema") is not None:
            self.ema.copy_(sd["ema"])
        self.step_count = sd["step"]
        self.param_groups[0]["lr"] = sd["lr"]


class FlatAdamW(_FlatTail):
    """AdamW over ddp.FlatParams.  `no_decay`: parameter names exempt from weight decay (see no_decay_names; every
    tensor starts on a 4-element granule of the flat buffer, so the exemption is one byte per granule)."""

    def __init__(self, flat, lr=5e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_norm=None, ema_decay=None,
                 no_decay=None, lr_scales=None):
        self.betas, self.eps = betas, eps
        self._setup(flat, lr, weight_decay, max_norm, ema_decay, no_decay, 3, lr_scales)

    def step(self):
        clip = self._begin_step(self._scalars)
        f = self.flat
        # f.grad_scale: 1 / world after the summing bucket all-reduce (ddp.BucketedGradReducer.finish) -- the mean of DDP
        if self.lr_scales is None:
            call("devit_adamw_step", ptr(f.flat), ptr(f.flat_grad), ptr(self.m), ptr(self.v), ptr(self.ema), ptr(f.flat16),
                 ptr(self.no_decay4), ptr(self.gnorm_sq) if clip else None, ptr(self._dyn), f.numel, self.betas[0], self.betas[1], self.eps,
                 self.weight_decay, float(self.max_norm or 0.0), float(self.ema_decay or 0.0), float(f.grad_scale),
                 stream_ptr())
        else:
            call("devit_adamw_step_lrs", ptr(f.flat), ptr(f.flat_grad), ptr(self.m), ptr(self.v), ptr(self.ema), ptr(f.flat16),
                 ptr(self.no_decay4), ptr(self.gnorm_sq) if clip else None, ptr(self._dyn), f.numel, self.betas[0], self.betas[1], self.eps,
                 self.weight_decay, float(self.max_norm or 0.0), float(self.ema_decay or 0.0), float(f.grad_scale),
                 ptr(self.lr_group4), ptr(self.lr_scales), stream_ptr())
        self._end_step()

    def state_dict(self):
        sd = super().state_dict()
        del sd["opt"]                           # AdamW's checkpoints carry no name (and load as AdamW: _check_kind)
        return sd


class FlatSGD(_FlatTail):
    """torch.optim.SGD(momentum, nesterov, dampening 0) over ddp.FlatParams with timm's two weight-decay groups: `--opt momentum` and
    `--opt nesterov` (devit_sgd_step)."""
    state_keys = ("buf",)

    def __init__(self, flat, lr=5e-4, momentum=0.9, nesterov=False, weight_decay=0.0, max_norm=None, ema_decay=None, no_decay=None,
                 lr_scales=None):
        self.momentum, self.nesterov = momentum, bool(nesterov)
        self.opt_name = "nesterov" if nesterov else "momentum"
        self._setup(flat, lr, weight_decay, max_norm, ema_decay, no_decay, 1, lr_scales)

    def step(self):
        clip = self._begin_step(lambda t: (self.param_groups[0]["lr"],))
        f = self.flat
        if self.lr_scales is None:
            call("devit_sgd_step", ptr(f.flat), ptr(f.flat_grad), ptr(self.buf), ptr(self.ema), ptr(f.flat16), ptr(self.no_decay4),
                 ptr(self.gnorm_sq) if clip else None, ptr(self._dyn), f.numel, self.momentum, int(self.nesterov),
                 self.weight_decay, float(self.max_norm or 0.0), float(self.ema_decay or 0.0), float(f.grad_scale), stream_ptr())
        else:
            call("devit_sgd_step_lrs", ptr(f.flat), ptr(f.flat_grad), ptr(self.buf), ptr(self.ema), ptr(f.flat16), ptr(self.no_decay4),
                 ptr(self.gnorm_sq) if clip else None, ptr(self._dyn), f.numel, self.momentum, int(self.nesterov),
                 self.weight_decay, float(self.max_norm or 0.0), float(self.ema_decay or 0.0), float(f.grad_scale),
                 ptr(self.lr_group4), ptr(self.lr_scales), stream_ptr())
        self._end_step()


class FlatAdam(_FlatTail):
    """torch.optim.Adam over ddp.FlatParams: the weight decay is L2, added to the gradient before the moments (`--opt adam`,
    devit_adam_l2_step)."""
    opt_name = "adam"

    def __init__(self, flat, lr=5e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_norm=None, ema_decay=None, no_decay=None,
                 lr_scales=None):
        self.betas, self.eps = betas, eps
        self._setup(flat, lr, weight_decay, max_norm, ema_decay, no_decay, 3, lr_scales)

    def step(self):
        clip = self._begin_step(self._scalars)
        f = self.flat
        if self.lr_scales is None:
            call("devit_adam_l2_step", ptr(f.flat), ptr(f.flat_grad), ptr(self.m), ptr(self.v), ptr(self.ema), ptr(f.flat16),
                 ptr(self.no_decay4), ptr(self.gnorm_sq) if clip else None, ptr(self._dyn), f.numel, self.betas[0], self.betas[1],
                 self.eps, self.weight_decay, float(self.max_norm or 0.0), float(self.ema_decay or 0.0), float(f.grad_scale),
                 stream_ptr())
        else:
            call("devit_adam_l2_step_lrs", ptr(f.flat), ptr(f.flat_grad), ptr(self.m), ptr(self.v), ptr(self.ema), ptr(f.flat16),
                 ptr(self.no_decay4), ptr(self.gnorm_sq) if clip else None, ptr(self._dyn), f.numel, self.betas[0], self.betas[1],
                 self.eps, self.weight_decay, float(self.max_norm or 0.0), float(self.ema_decay or 0.0), float(f.grad_scale),
                 ptr(self.lr_group4), ptr(self.lr_scales), stream_ptr())
        self._end_step()


def lamb_chunk_table(names, sizes, offsets, no_decay, chunk_granules=L.OPT_CHUNK_GRANULES):
    """The devit_opt_chunk table of a flat buffer, an int32 CPU tensor [nchunks][4] (first granule, granule count, segment, flags): tensor s
    (names[s], sizes[s] elements from offsets[s], a multiple of 4) is cut into chunks of at most `chunk_granules` granules, in order;
    flags bit 0 marks the tensors in `no_decay`.  The padding between tensors belongs to no chunk."""
    rows = []
    for s, (name, numel, off) in enumerate(zip(names, sizes, offsets)):
        if off % 4:
            raise ValueError(f"{name}: offset {off} is not on a 4-element granule")
        first, count = off // 4, (numel + 3) // 4
        flag = L.OPT_CHUNK_NO_DECAY if name in no_decay else 0
        for c in range(0, count, chunk_granules):
            rows.append((first + c, min(chunk_granules, count - c), s, flag))
    return torch.tensor(rows, dtype=torch.int32).reshape(-1, 4)


def validate_chunk_table(table, sizes, offsets, numel, chunk_granules=L.OPT_CHUNK_GRANULES):
    """Raise ValueError unless `table` (lamb_chunk_table's layout) is what the kernels may trust: every chunk inside [0, numel / 4) and
    inside the tensor it names, at most `chunk_granules` long, the chunks disjoint and sorted by segment, one flag per tensor, and
    every granule of every tensor covered exactly once.  The kernels index the buffers with these numbers."""
    t = table.to(torch.int64)
    if t.ndim != 2 or t.shape[1] != 4 or t.shape[0] == 0:
        raise ValueError("chunk table: expected [nchunks > 0][4]")
    first, count, seg, flags = t.unbind(1)
    if bool((first < 0).any()) or bool((count < 1).any()) or bool((count > chunk_granules).any()) or bool((first + count > numel // 4).any()):
        raise ValueError("chunk table: a chunk is empty, longer than a chunk may be, or outside the flat buffer")
    if bool((seg < 0).any()) or bool((seg >= len(sizes)).any()) or bool((seg[1:] < seg[:-1]).any()):
        raise ValueError("chunk table: a segment index is out of range, or the table is not sorted by segment")
    lo = torch.tensor([o // 4 for o in offsets])[seg]
    hi = torch.tensor([(o + n + 3) // 4 for o, n in zip(offsets, sizes)])[seg]
    if bool((first < lo).any()) or bool((first + count > hi).any()):
        raise ValueError("chunk table: a chunk reaches outside its tensor")
    covered = torch.zeros(numel // 4 + 1, dtype=torch.int64)
    covered.index_add_(0, first, torch.ones_like(first))
    covered.index_add_(0, first + count, -torch.ones_like(first))
    covered = covered.cumsum(0)[:-1]
    want = torch.zeros(numel // 4, dtype=torch.int64)
    for o, n in zip(offsets, sizes):
        want[o // 4:(o + n + 3) // 4] += 1
    if bool((covered > 1).any()):
        raise ValueError("chunk table: chunks overlap")
    if not torch.equal(covered, want):
        raise ValueError("chunk table: a granule of a tensor is not covered, or padding is")
    per_seg = {}
    for s, f in zip(seg.tolist(), flags.tolist()):
        if per_seg.setdefault(s, f) != f:
            raise ValueError(f"chunk table: the chunks of tensor {s} disagree on their flags")
    return table


class FlatLamb(_FlatTail):
    """timm Lamb (bias_correction, grad_averaging, max_grad_norm = 1, always_adapt off) over ddp.FlatParams: `--opt lamb`, and `--opt lambc`
    with trust_clip.  The trust ratio is per parameter tensor: the flat buffer is described to devit_lamb_step by a chunk table built
    (and validated) here once.  Tensors of the no-decay group -- all of them when weight_decay is 0 -- take trust 1, as in timm."""

    def __init__(self, flat, lr=5e-4, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.0, max_norm=None, ema_decay=None, no_decay=None,
                 trust_clip=False, lr_scales=None):
        self.betas, self.eps, self.trust_clip = betas, eps, bool(trust_clip)
        self.opt_name = "lambc" if trust_clip else "lamb"
        self._setup(flat, lr, weight_decay, max_norm, ema_decay, no_decay, 3, lr_scales)
        sizes = [p.numel() for p in flat.params]
        exempt = set(flat.names) if not weight_decay else set(no_decay or ())
        self.chunks_host = validate_chunk_table(lamb_chunk_table(flat.names, sizes, flat.offsets, exempt), sizes, flat.offsets, flat.numel)
        dev = flat.flat.device
        self.nchunks, self.nsegments = self.chunks_host.shape[0], len(sizes)
        self.chunks = self.chunks_host.to(dev)
        self._lamb_ws = torch.empty((2 * self.nchunks + self.nsegments) * 4, dtype=torch.uint8, device=dev)

    def trust(self):
        """the trust ratios of the last step, one per tensor of flat.names (1 for the no-decay group)"""
        return self._lamb_ws.view(torch.float32)[2 * self.nchunks:]

    def step(self):
        self._begin_step(self._scalars, need_norm=True)
        f = self.flat
        if self.lr_scales is None:
            call("devit_lamb_step", ptr(f.flat), ptr(f.flat_grad), ptr(self.m), ptr(self.v), ptr(self.ema), ptr(f.flat16),
                 ptr(self.gnorm_sq), ptr(self._dyn), f.numel, ptr(self.chunks), self.nchunks, self.nsegments, int(self.trust_clip),
                 self.betas[0], self.betas[1], self.eps, self.weight_decay, float(self.max_norm or 0.0), float(self.ema_decay or 0.0),
                 float(f.grad_scale), ptr(self._lamb_ws), self._lamb_ws.numel(), stream_ptr())
        else:
            call("devit_lamb_step_lrs", ptr(f.flat), ptr(f.flat_grad), ptr(self.m), ptr(self.v), ptr(self.ema), ptr(f.flat16),
                 ptr(self.gnorm_sq), ptr(self._dyn), f.numel, ptr(self.chunks), self.nchunks, self.nsegments, int(self.trust_clip),
                 self.betas[0], self.betas[1], self.eps, self.weight_decay, float(self.max_norm or 0.0), float(self.ema_decay or 0.0),
                 float(f.grad_scale), ptr(self._lamb_ws), self._lamb_ws.numel(), ptr(self.lr_group4), ptr(self.lr_scales), stream_ptr())
        self._end_step()


def check_layer_decay(decay):
    """`--layer-decay D`: None (absent) or a number in (0, 1]; SystemExit otherwise"""
    if decay is not None and not (math.isfinite(decay) and 0.0 < decay <= 1.0):
        raise SystemExit(f"--layer-decay {decay}: the decay per layer lies in (0, 1] (1 trains every layer at the scheduled lr)")


def create_flat_optimizer(args, flat, model, layer_decay=True):
    """timm create_optimizer(args, model) for the fused tails: `--opt` (adamw, adam, momentum, nesterov, lamb, lambc), `--momentum`,
    `--opt-eps`, `--opt-betas`, `--weight-decay`, `--clip-grad`, `--model-ema` / `--model-ema-decay` -> the optimizer over `flat`, with
    timm's two weight-decay groups of `model`.  `--layer-decay D` below 1 gives every tensor the learning rate of its depth (layer_decay_scales
    over model_depth(model); one line per layer id is printed); layer_decay=False: this optimizer ignores the flag (the ensemble's fusion head)."""
    name = args.opt.lower()
    if name not in OPT_NAMES:
        raise ValueError(f"--opt {args.opt}: not one of {', '.join(OPT_NAMES)}")
    kw = dict(lr=args.lr, weight_decay=args.weight_decay, max_norm=args.clip_grad,
              ema_decay=args.model_ema_decay if getattr(args, "model_ema", False) else None, no_decay=no_decay_names(model))
    decay = getattr(args, "layer_decay", None) if layer_decay else None
    check_layer_decay(decay)
    if decay is not None and decay != 1.0:      # 1.0 is the unscaled path: the old entry points, their bits
        depth = model_depth(model)
        kw["lr_scales"] = layer_decay_scales(flat.names, depth, decay)
        ids = layer_ids(flat.names, depth)
        for i in range(depth + 2):
            print(f"--layer-decay {decay}: layer {i:2d}  lr x {float(decay) ** (depth + 1 - i):.6g}  {sum(1 for v in ids.values() if v == i)} tensors")
    adam = dict(eps=args.opt_eps, betas=tuple(args.opt_betas or (0.9, 0.999)), **kw)
    if name in ("momentum", "nesterov"):
        opt = FlatSGD(flat, momentum=args.momentum, nesterov=name == "nesterov", **kw)
    elif name == "adamw":
        opt = FlatAdamW(flat, **adam)
    elif name == "adam":
        opt = FlatAdam(flat, **adam)
    else:
        opt = FlatLamb(flat, trust_clip=name == "lambc", **adam)
    if "lr_scales" in kw:
        opt.layer_decay = float(decay)
    return opt
