"""Step loops with the reference's names and semantics (engine.py), hosted on the HIP path.

  distill_forward   : engine.py:68-106 (student train forward, teacher eval forward, DEKD losses)
  train_1epoch_qkv  : engine.py:48-140
  evaluate          : engine.py:17-45
The five `.item()` host syncs + `cuda.synchronize()` per step of the reference (engine.py:108-117,130) are
kept for logging parity in train_1epoch_qkv, but only every `print_freq` steps.
"""
import math
import operator
import os
import sys

import torch

from . import de_vit, losses, ops


def _hand_over(out, main):
    """Outputs of a side-stream forward that the main stream will read.  Small tensors from the side stream's allocator
    pool are marked with record_stream(); the packed qkv buffers of the composite path are views of an arena that was
    allocated from the MAIN stream's pool (ops.ARENA_ALLOC_STREAM) and need no mark -- see the note there."""
    o = out['output']
    for t in (o if isinstance(o, tuple) else (o,)):
        t.record_stream(main)
    for qkv in out['qkv']:
        if qkv is None:
            continue
        packed = getattr(qkv[0], "_devit_packed", (qkv[0],))[0]
        if getattr(packed, "_devit_arena", False):
            continue                      # tagged by the composite path: lives in the main stream's pool already
        if packed.untyped_storage().nbytes() <= packed.numel() * packed.element_size():    # its own allocation
            packed.record_stream(main)
    for t in out.get('encoder') or ():    # (hid_gama > 0: the selected blocks' hidden states -- views of their arenas on the 16-bit path, as the qkv buffers; a last block's is a clone)
        if t is not None and t.untyped_storage().nbytes() <= t.numel() * t.element_size():
            t.record_stream(main)


RELATION_WORDS = ("mid", "last", "all")


def resolve_relation_layers(spec, student_depth, teacher_depth):
    """The layer pairs ((s, t), ...) whose q/k/v (and, with the other families on, hidden states) the step compares -- --relation-layers.
    spec: None or "mid" (the reference's one pair, engine.py:91-92: block depth // 2 - 1 of each model), "last", "all", or an iterable of 0-based
    student block indices (sorted, deduplicated).  The teacher's block of student block s is t(s) = (s + 1) * (tl // sl) - 1: the last block of
    the s-th of sl equal groups of teacher blocks, which is the reference's pair for "mid" at every depth ratio.  ValueError names the offender."""
    sl, tl = int(student_depth), int(teacher_depth)
    if sl < 1 or tl < 1 or tl % sl != 0:
        raise ValueError(f"relation layers: the teacher's depth {tl} is not a multiple of the student's depth {sl}: the layers cannot be paired")
    if isinstance(spec, (list, tuple)) and len(spec) == 1 and isinstance(spec[0], str) and not spec[0].lstrip("+-").isdigit():
        spec = spec[0]                             # (the command line's one word)
    if spec is None:
        spec = "mid"
    if isinstance(spec, str):
        if spec not in RELATION_WORDS:
            raise ValueError(f"relation layers: unknown selection {spec!r}: one of {', '.join(RELATION_WORDS)}, or 0-based student block indices")
        if spec == "mid" and sl < 2:
            raise ValueError(f"relation layers: 'mid' is block depth // 2 - 1: a student of depth {sl} has none")
        layers = {"mid": [sl // 2 - 1], "last": [sl - 1], "all": list(range(sl))}[spec]
    else:
        layers = []
        for v in spec:
            try:                                   # (the command line hands the indices over as strings)
                i = int(v, 10) if isinstance(v, str) else operator.index(v)
            except (ValueError, TypeError):
                raise ValueError(f"relation layers: {v!r} is not a 0-based student block index"
                                 + (f": {v!r} stands alone, not among indices" if v in RELATION_WORDS else "")) from None
            if i < 0 or i >= sl:
                raise ValueError(f"relation layers: block index {i} is outside the student's blocks 0 .. {sl - 1}")
            layers.append(i)
        if not layers:
            raise ValueError("relation layers: the selection [] is empty: name at least one student block")
        layers = sorted(set(layers))
    r = tl // sl
    return tuple((s, (s + 1) * r - 1) for s in layers)


def _unwrapped(m):
    return m.module if hasattr(m, "module") else m


def _depth(m):
    m = _unwrapped(m)
    return len(m.blocks) if hasattr(m, "blocks") else None


def _request(m, layers, hid):
    """What the next forwards of `m` hand out beside the logits: the q/k/v of `layers` with the zeroed overhang rows the relation kernels read
    (qkv_pad_layers) and, with `hid`, those blocks' 'encoder' outputs.  Set on every call: the request follows the step's selection, it does not
    stick to the model.  A selection that holds the last block makes the model run it in full (de_vit.run_blocks drops the lean tail)."""
    vit = _unwrapped(m)
    vit._rel_request = frozenset(layers)
    vit._hid_request = bool(hid)
    if hasattr(vit, "blocks"):
        vit.qkv_pad_layers = set(layers)


def _hid_layers(vit):
    """The blocks whose output enters the hidden-state relation loss: those whose q/k/v enter the relation losses (engine.py:91-92: the middle one)."""
    return set(getattr(vit, "_rel_request", None) or {len(vit.blocks) // 2 - 1})


def _forward_outputs(m, samples):
    """m(samples) with the outputs the step reads: q/k/v, and -- when the step asked for it (m._hid_request, set by distill_forward /
    TeacherLookahead for hid_gama > 0) -- the 'encoder' outputs of the selected blocks alone (enc_layers), which keeps the lean tail unless the
    last block is one of them."""
    vit = _unwrapped(m)
    if not getattr(vit, "_hid_request", False):
        return m(samples, output_qkv=True)
    prev, vit.enc_layers = getattr(vit, "enc_layers", None), _hid_layers(vit)
    try:
        return m(samples, output_qkv=True, output_encoders=True)
    finally:
        vit.enc_layers = prev


def _side_forward(teacher_model, samples, main, side):
    side.wait_stream(main)
    prev, ops.ARENA_ALLOC_STREAM = ops.ARENA_ALLOC_STREAM, main
    try:
        with torch.cuda.stream(side), torch.no_grad(), de_vit.lean_tail(teacher_model):
            return _forward_outputs(teacher_model, samples)
    finally:
        ops.ARENA_ALLOC_STREAM = prev


def distill_forward(model, teacher_model, samples, targets, gama=(0.2, 0.1, 0.3), kind="hard", alpha=0.5, tau=1.0,
                    criterion=None, dp_scales="draw", teacher_outputs=None, after_student=None, hid_gama=0.0, qkv_ce_gama=0.0,
                    qkv_cross_gama=0.0, qkv_layout="view", relation_layers=None):
    """One DEKD forward.  Returns dict(loss, cls_loss, q_loss, k_loss, v_loss, logits, teacher_logits).
    teacher_outputs: the teacher's outputs for `samples` if they were computed ahead (TeacherLookahead).
    after_student: called once the student's forward is enqueued (TeacherLookahead.launch of the NEXT batch).
    hid_gama > 0: loss += hid_gama * cal_hid_relation_loss of the middle blocks' hidden states (utils/losses.py:295-304; the layer pair the q/k/v
    relation losses use), returned as `hid_loss`; student and teacher then hand out that one block's 'encoder' output (enc_layers).  0: the step as
    it was, dict and all.
    qkv_ce_gama / qkv_cross_gama > 0: loss += qkv_ce_gama * cal_qkv_loss([s_mid], [t_mid]) + qkv_cross_gama * cal_qkv_loss2([s_mid], [t_mid])
    (utils/losses.py:247-292) on the same middle layer pair, rows per qkv_layout; returned as `qkv_ce_loss` / `qkv_cross_loss`.  Both 0: the step
    as it was, dict and all.
    relation_layers: the layer pairs all of the above compare (resolve_relation_layers: None or "mid", "last", "all", student block indices) in
    place of "the middle pair": loss = cls + sum over the pairs of sum_j gama_j * relation_loss_j(s, t) / depth_s + the list losses over the pairs'
    lists, each with the reference's own normalisation (/ len, / 3 len, / 9 len).  q_loss / k_loss / v_loss are the sums over the pairs / depth_s;
    `rel_layers` is the [len(pairs), 3] tensor of the unscaled per-pair losses.  None: the step as it was, dict and all (no `rel_layers`); its
    numbers are those of "mid".  The models' requests (qkv_pad_layers, the hidden states handed out, the lean tail) follow the selection on
    every call; teacher outputs computed ahead for another selection are a RuntimeError."""
    vit = model.module if hasattr(model, "module") else model
    hid_gama = float(hid_gama)
    if not hid_gama >= 0.:
        raise ValueError(f"hid_gama must be >= 0, got {hid_gama}")
    qkv_ce_gama, qkv_cross_gama = float(qkv_ce_gama), float(qkv_cross_gama)
    for name, w in (("qkv_ce_gama", qkv_ce_gama), ("qkv_cross_gama", qkv_cross_gama)):
        if not w >= 0.:
            raise ValueError(f"{name} must be >= 0, got {w}")
    if qkv_layout not in ops.QKV_LAYOUTS:
        raise ValueError(f"qkv_layout must be one of {sorted(ops.QKV_LAYOUTS)}, got {qkv_layout!r}")
    hid = hid_gama > 0.
    tvit = _unwrapped(teacher_model)
    # the selection, resolved before the forwards when both depths are known from the models (else from the outputs, below)
    pairs = None
    if _depth(vit) is not None and _depth(tvit) is not None:
        pairs = resolve_relation_layers(relation_layers, _depth(vit), _depth(tvit))
    if pairs is not None and teacher_outputs is not None:
        _check_teacher_outputs(teacher_outputs, pairs)
    # only the selected blocks' q/k/v enter the relation loss (engine.py:91-100: the middle one): the other blocks' packed qkv buffers need no
    # zeroed overhang rows.  The request is made on every call -- a selection does not stick to the model object.
    if pairs is not None:
        _check_compacted(vit, pairs)
        _request(vit, [s for s, _ in pairs], hid)
        if teacher_outputs is None:      # (a TeacherLookahead makes its request when it launches)
            _request(tvit, [t for _, t in pairs], hid)
    else:
        vit._hid_request = hid
        if teacher_outputs is None:
            tvit._hid_request = hid
    pre_teacher = None
    if teacher_outputs is None and os.environ.get("DEVIT_TEACHER_STREAM", "1") == "1" and samples.is_cuda:
        pre_teacher = _teacher_forward_async(teacher_model, samples)
    # only the logits and the selected blocks' q/k/v are read below: unless the last block is one of them it runs on its two token rows
    # (de_vit.lean_tail)
    with de_vit.lean_tail(vit):
        if dp_scales != "draw":   # explicit DropPath masks (parity tests)
            outputs = _forward_with_dp(vit, samples, dp_scales, hid)
        else:
            outputs = _forward_outputs(model, samples)                              # engine.py:70
    logits, qkvs = outputs['output'], outputs['qkv']
    if after_student is not None:
        after_student()
    if teacher_outputs is None:                                                     # engine.py:73-76
        teacher_outputs = pre_teacher() if pre_teacher is not None else _teacher_forward(teacher_model, samples)
    teacher_logits, teacher_qkvs = teacher_outputs['output'], teacher_outputs['qkv']
    if criterion is None:
        criterion = losses.DistillLoss(losses.SoftTargetCrossEntropy(), kind, alpha, tau)
    cls_loss = criterion(outputs=logits, teacher_outputs=teacher_logits, labels=targets)   # :79
    tl, sl = len(teacher_qkvs), len(qkvs)
    if pairs is None:
        pairs = resolve_relation_layers(relation_layers, sl, tl)
    _check_outputs(outputs, teacher_outputs, pairs, hid)
    s_qkvs, t_qkvs = [qkvs[s] for s, _ in pairs], [teacher_qkvs[t] for _, t in pairs]
    rel3 = losses.relation_losses_vector(s_qkvs[0], t_qkvs[0])                             # :91-100, as one [q, k, v] tensor
    if rel3 is not None:
        # :102-106 on the vector: total = cls + sum_j (gama_j / sl) loss_j (one multiply-sum + one add; backward one multiply) and the
        # three logged values as views of loss / sl -- the scalar form costs ~25 tiny kernels per step around the same numbers
        if len(pairs) == 1:
            rel, summed = rel3, rel3
        else:            # one [L, 3] tensor of the pairs' losses: the weights broadcast over its rows, the logged values are its column sums
            rel = torch.stack([rel3] + [losses.relation_losses_vector(sq, tq) for sq, tq in zip(s_qkvs[1:], t_qkvs[1:])])
            summed = rel.sum(0)
        scaled = summed / sl
        q_loss, k_loss, v_loss = scaled[0], scaled[1], scaled[2]
        # (an elementwise product + sum, not torch.dot: on ROCm torch.dot is a rocBLAS call, and no vendor BLAS runs on this path)
        loss = cls_loss + (rel * _relation_weights(gama, sl, rel.device)).sum()
        rel_layers = rel.detach().view(len(pairs), 3)
    else:
        per = [losses.relation_losses_packed(sq, tq) for sq, tq in zip(s_qkvs, t_qkvs)]
        q_loss, k_loss, v_loss = (sum(p[j] for p in per) / sl for j in range(3))        # :102-104
        loss = cls_loss + float(gama[0]) * q_loss + float(gama[1]) * k_loss + float(gama[2]) * v_loss   # :105-106
        rel_layers = torch.stack([torch.stack([x.detach() for x in p]) for p in per])
    out = dict(loss=loss, cls_loss=cls_loss, q_loss=q_loss, k_loss=k_loss, v_loss=v_loss, logits=logits,
               teacher_logits=teacher_logits)
    if relation_layers is not None:      # (None: the step as it was, dict and all)
        out['rel_layers'] = rel_layers
    if hid:
        s_enc, t_enc = outputs['encoder'], teacher_outputs['encoder']
        out['hid_loss'] = losses.cal_hid_relation_loss([s_enc[s] for s, _ in pairs], [t_enc[t] for _, t in pairs],
                                                       exact=getattr(vit, "precision", "bf16") == "f32")
        out['loss'] = loss + hid_gama * out['hid_loss']
    if qkv_ce_gama > 0.:
        out['qkv_ce_loss'] = losses.cal_qkv_loss(s_qkvs, t_qkvs, layout=qkv_layout)
        out['loss'] = out['loss'] + qkv_ce_gama * out['qkv_ce_loss']
    if qkv_cross_gama > 0.:
        out['qkv_cross_loss'] = losses.cal_qkv_loss2(s_qkvs, t_qkvs, layout=qkv_layout)
        out['loss'] = out['loss'] + qkv_cross_gama * out['qkv_cross_loss']
    return out


def _check_compacted(vit, pairs):
    """A student compacted for training keeps every head in the GEMMs of the blocks whose q/k/v enter the relation losses (a masked head's q/k/v
    still do, shrink.compact): refuse a selection whose block has lost them instead of comparing fewer heads in silence."""
    for s, _ in pairs:
        blk = vit.blocks[s]
        c = getattr(blk, "_compact", None)
        if c is not None and c.get("heads_compacted") and c["num_heads"] < blk.attn.num_heads:
            raise RuntimeError(f"distill_forward: block {s} of the student is one of this step's relation layers {[p[0] for p in pairs]}, but it was "
                               f"compacted to {c['num_heads']} of its {blk.attn.num_heads} heads: the q/k/v of its masked heads enter the relation "
                               "losses -- compact with shrink.compact(model, trainable=True, relation_layers=...) for the step's selection")


def _selection_text(pairs):
    return "student blocks %s / teacher blocks %s" % ([s for s, _ in pairs], [t for _, t in pairs])


def _check_teacher_outputs(teacher_outputs, pairs):
    """Teacher outputs computed ahead carry the teacher blocks they were prepared for (TeacherLookahead.take): refuse another selection's."""
    made = teacher_outputs.get('relation_layers') if isinstance(teacher_outputs, dict) else None
    want = tuple(t for _, t in pairs)
    if made is not None and tuple(made) != want:
        raise RuntimeError(f"distill_forward: this step's relation layers are {_selection_text(pairs)}, the teacher outputs handed in were computed "
                           f"ahead for teacher blocks {list(made)}: build the look-ahead for the step's selection, "
                           "TeacherLookahead(teacher, relation_layers=..., student_depth=...)")


def _check_outputs(outputs, teacher_outputs, pairs, hid):
    """Every entry the losses read is there -- a RuntimeError here, not a failure inside a loss."""
    _check_teacher_outputs(teacher_outputs, pairs)
    made = teacher_outputs.get('relation_layers') if isinstance(teacher_outputs, dict) else None
    made = "" if made is None else f" (computed ahead for teacher blocks {list(made)})"
    for who, o, idx in (("student's", outputs, [s for s, _ in pairs]), ("teacher's", teacher_outputs, [t for _, t in pairs])):
        qk = o['qkv']
        gone = [i for i in idx if i >= len(qk) or qk[i] is None]
        if gone:
            raise RuntimeError(f"distill_forward: this step's relation layers are {_selection_text(pairs)}, but the {who} outputs"
                               f"{made if who[0] == 't' else ''} hold no q/k/v of block(s) {gone} -- a forward inside de_vit.lean_tail hands out "
                               "none of its last block unless that block was requested")
        if hid:
            enc = o.get('encoder')
            gone = [i for i in idx if not enc or i >= len(enc) or enc[i] is None]
            if gone:
                raise RuntimeError(f"distill_forward(hid_gama > 0): this step's relation layers are {_selection_text(pairs)}, but the {who} outputs"
                                   f"{made if who[0] == 't' else ''} hold no hidden states of block(s) {gone} -- teacher outputs computed ahead "
                                   "must come from TeacherLookahead(teacher, hid=True, relation_layers=...)")


_side_stream = {}
_rel_w = {}


def _relation_weights(gama, layers, device):
    """[gama_q, gama_k, gama_v] / layers as a cached device tensor."""
    key = (float(gama[0]), float(gama[1]), float(gama[2]), int(layers), str(device))
    w = _rel_w.get(key)
    if w is None:
        w = _rel_w[key] = torch.tensor([key[0] / layers, key[1] / layers, key[2] / layers], dtype=torch.float32, device=device)
    return w


def _teacher_forward(teacher_model, samples):
    """Frozen teacher forward.  With DEVIT_TEACHER_STREAM=1 it is enqueued on a side stream before the student
    forward has drained, so the tail rounds of one model's GEMMs are filled by the other's workgroups."""
    if os.environ.get("DEVIT_TEACHER_STREAM", "1") != "1" or not samples.is_cuda:
        with torch.no_grad(), de_vit.lean_tail(teacher_model):
            return _forward_outputs(teacher_model, samples)
    main = torch.cuda.current_stream()
    side = _side_stream.setdefault(samples.device.index, torch.cuda.Stream())
    out = _side_forward(teacher_model, samples, main, side)   # NOTE: call BEFORE the student forward is enqueued to overlap
    main.wait_stream(side)
    _hand_over(out, main)
    return out


def _teacher_forward_async(teacher_model, samples):
    """Enqueue the teacher forward on the side stream now; the returned callable joins it."""
    main = torch.cuda.current_stream()
    side = _side_stream.setdefault(samples.device.index, torch.cuda.Stream())
    out = _side_forward(teacher_model, samples, main, side)

    def join():
        main.wait_stream(side)
        _hand_over(out, main)
        return out
    return join


def row_dtypes_for(*models):
    """The 16-bit patch-row types one im2row pass must produce so that every model of the step can read it (ops.patch_rows(dtypes=...)); None when
    a model runs the exact-fp32 kernels (they read the images themselves) or is not on a GPU."""
    out = []
    for m in models:
        if m is None:
            continue
        prec = getattr(m, "precision", "bf16")
        if prec == "f32" or not any(p.is_cuda for p in m.parameters()):
            return None
        dt = torch.float16 if prec == "f16" else torch.bfloat16
        if dt not in out:
            out.append(dt)
    return tuple(out) or None


class TeacherLookahead:
    """Frozen-teacher forward one batch ahead (engine.py:73-76 computes it inside the step).

    The teacher has no dependence on the student, so its forward for batch k+1 can be enqueued on the side stream as
    soon as batch k+1 exists: it then runs beside the student's backward of batch k, and the workgroups of one model
    fill the partial last rounds of the other's kernels for the whole step, not only during the student forward.
    Same arithmetic per step; one batch of teacher outputs (logits + one block's q/k/v) stays resident.

        look = TeacherLookahead(teacher); look.submit(batch0)
        for k: t_out = look.take(batch_k); look.submit(batch_k+1); distill_forward(..., batch_k, teacher_outputs=t_out)
    """

    layers, hid = None, None     # (an object made without __init__ prepares nothing and stamps nothing)

    def __init__(self, teacher_model, hid=False, relation_layers=None, student_depth=None):
        """hid: the forwards also hand out the selected blocks' hidden states (distill_forward(hid_gama > 0) reads them).
        relation_layers, student_depth: the step's selection (resolve_relation_layers) and the depth of the student it is paired with (None: the
        teacher's own depth); the forwards are prepared for the teacher side of the pairs, and the outputs carry it ('relation_layers') so that a
        step with another selection refuses them.  None: the middle block."""
        self.teacher = teacher_model
        self.hid = bool(hid)
        depth = _depth(teacher_model)
        if depth is not None:
            pairs = resolve_relation_layers(relation_layers, depth if student_depth is None else student_depth, depth)
            self.layers = tuple(t for _, t in pairs)
        elif relation_layers is None:
            self.layers = None
        else:
            raise ValueError("TeacherLookahead(relation_layers=...): the teacher has no `blocks` to select from")
        self._prepare()
        self._pending = None

    def _prepare(self):
        """the teacher's request, made again at every launch: a step run in between with another selection (or none ahead) leaves its own behind"""
        if self.hid is None:
            return
        if self.layers is not None:
            _request(self.teacher, self.layers, self.hid)
        else:
            _unwrapped(self.teacher)._hid_request = self.hid

    def submit(self, samples, defer=False):
        """defer: record the batch, enqueue its forward at launch() (or at take(), at the latest).  Round 6: the loop launches the NEXT batch's
        teacher forward behind the student's forward of the current one (distill_forward(after_student=...)) instead of in front of it: the side
        stream then starts when the student forward has drained, and the teacher runs beside the backward -- whose launches leave CUs idle (198-tile
        dgrads, attention, LayerNorm) -- and the next forward's first half, not beside a forward of CU-filling GEMMs that it only delays.  Same
        arithmetic, +0.9 % (three interleaved pairs: 11372 / 11407 / 11395 -> 11487 / 11488 / 11552 img/s).  DEVIT_TEACHER_SUBMIT=early: as before."""
        if self._pending is not None:
            raise RuntimeError("TeacherLookahead.submit: the previous batch was not taken")
        self._pending = [samples, None]
        if not defer or os.environ.get("DEVIT_TEACHER_SUBMIT", "late") == "early":
            self.launch()

    def launch(self):
        if self._pending is not None and self._pending[1] is None:
            self._prepare()
            self._pending[1] = _teacher_forward_async(self.teacher, self._pending[0])

    def take(self, samples):
        if self._pending is None or self._pending[0] is not samples:
            raise RuntimeError("TeacherLookahead.take: not the batch that was submitted")
        self.launch()
        join, self._pending = self._pending[1], None
        out = join()
        if self.layers is not None and isinstance(out, dict):
            out['relation_layers'] = self.layers
        return out


class _PreparedBatches:
    """data_loader -> (samples on device after mixup, targets, teacher outputs or None), one batch ahead when a
    TeacherLookahead is given (engine.py:62-68 does the transfer + mixup at the top of each iteration)."""

    def __init__(self, loader, device, mixup_fn, look, row_dtypes=None):
        self.loader, self.device, self.mixup_fn, self.look = loader, device, mixup_fn, look
        # 16-bit types of the patch rows the step's models read (row_dtypes_for): a batch that arrives as fp32 images (no device mixup) is cut
        # into patch rows ONCE here, and the student and the look-ahead teacher share them, as they share the mixed rows when mixup is on
        self.row_dtypes = row_dtypes
        self._h2d = None

    def __len__(self):
        return len(self.loader)

    def _to_device(self, samples, targets):
        """Host batches cross PCIe on a copy stream of their own (154 MB per bs-256 batch, ~3 ms): _prep runs one
        batch ahead of the step that consumes it, and the host enqueues ahead of the GPU, so the copy lands under the
        previous step's kernels instead of in front of this one's (pinned source memory assumed for that)."""
        dev = torch.device(self.device)
        if dev.type != "cuda" or (samples.device.type != "cpu" and targets.device.type != "cpu"):
            return samples.to(dev, non_blocking=True), targets.to(dev, non_blocking=True)
        if self._h2d is None:
            self._h2d = torch.cuda.Stream(device=dev)
        main = torch.cuda.current_stream(dev)
        with torch.cuda.stream(self._h2d):
            samples = samples.to(dev, non_blocking=True)
            targets = targets.to(dev, non_blocking=True)
        main.wait_stream(self._h2d)
        for t in (samples, targets):
            t.record_stream(main)
        return samples, targets

    def _prep(self, batch):
        samples, targets = batch
        samples, targets = self._to_device(samples, targets)
        if self.mixup_fn is not None:
            samples, targets = self.mixup_fn(samples, targets)
        if self.row_dtypes and isinstance(samples, torch.Tensor) and samples.is_cuda and samples.dim() == 4:
            samples = ops.patch_rows(samples, dtypes=self.row_dtypes)
        return samples, targets

    def launch_teacher(self):
        """distill_forward(after_student=...): the student's forward of the current batch is enqueued -- now the next batch's teacher forward"""
        if self.look is not None:
            self.look.launch()

    def __iter__(self):
        it = iter(self.loader)
        cur = next(it, None)
        if cur is None:
            return
        cur = self._prep(cur)
        if self.look is not None:
            self.look.submit(cur[0])
        while cur is not None:
            nxt = next(it, None)
            nxt = self._prep(nxt) if nxt is not None else None
            t_out = None
            if self.look is not None:
                t_out = self.look.take(cur[0])
                if nxt is not None:
                    self.look.submit(nxt[0], defer=True)      # launched by launch_teacher() behind the student's forward, or by the next take()
            yield cur[0], cur[1], t_out
            cur = nxt


def _forward_with_dp(vit, samples, dp_scales, hid=False):
    x = vit.embed(samples)
    xo, qkvs, _, encs = de_vit.run_blocks(list(vit.blocks), x, vit.training, True, False, hid,
                                          grad_ready=vit.grad_ready, dp_scales=dp_scales, precision=vit.precision,
                                          qkv_pad_layers=getattr(vit, "qkv_pad_layers", None),
                                          lean_tokens=vit.num_tokens if getattr(vit, "_lean_tail", False) else 0,
                                          enc_layers=_hid_layers(vit) if hid else None)
    heads = vit._tokens_and_logits(xo, True)
    return {'output': (heads[1], heads[2]) if vit.training else (heads[1] + heads[2]) / 2, 'qkv': qkvs, 'encoder': encs}


def train_1epoch_qkv(model, teacher_model, criterion, data_loader, optimizer, device, epoch, loss_scaler, log, args,
                     max_norm=0, model_ema=None, mixup_fn=None, print_freq=10):
    """engine.py:48-140.  `loss_scaler(loss, optimizer, clip_grad=, parameters=)` keeps timm NativeScaler's call
    shape; bf16 needs no loss scaling, so devit_amd.optim.StepRunner is the usual object here."""
    from .utils import MetricLogger, SmoothedValue
    model.train(True)
    metric_logger = MetricLogger(delimiter="  ")
    hid_gama = float(getattr(args, "hid_gama", 0.0) or 0.0)        # --hid-gama: the hidden-state relation term (0: the step and its log line as they were)
    # --qkv-ce-gama / --qkv-cross-gama / --qkv-layout: the soft cross-entropy relation terms (0: the step and its log line as they were)
    qkv_ce_gama, qkv_cross_gama = float(getattr(args, "qkv_ce_gama", 0.0) or 0.0), float(getattr(args, "qkv_cross_gama", 0.0) or 0.0)
    qkv_layout = getattr(args, "qkv_layout", "view") or "view"
    extra = [n for n, w in (('hid_loss', hid_gama), ('qkv_ce_loss', qkv_ce_gama), ('qkv_cross_loss', qkv_cross_gama)) if w > 0]
    for name in ('lr', 'cls_loss', 'q_loss', 'k_loss', 'v_loss') + tuple(extra):
        metric_logger.add_meter(name, SmoothedValue(window_size=1, fmt='{value:.6f}'))
    header = 'Epoch: [{}]'.format(epoch)
    step = 0
    lookahead = bool(getattr(args, "teacher_lookahead", True)) and device is not None and str(device).startswith("cuda")
    relation_layers = getattr(args, "relation_layers", None)       # --relation-layers: the layer pairs of all relation terms (None: the middle pair)
    look = TeacherLookahead(teacher_model, hid=hid_gama > 0, relation_layers=relation_layers, student_depth=_depth(model)) if lookahead else None
    batches = _PreparedBatches(data_loader, device, mixup_fn, look, row_dtypes=row_dtypes_for(model, teacher_model))
    for samples, targets, teacher_out in metric_logger.log_every(batches, print_freq, header):
        out = distill_forward(model, teacher_model, samples, targets, gama=args.gama, criterion=criterion,
                              teacher_outputs=teacher_out, after_student=batches.launch_teacher, hid_gama=hid_gama,
                              qkv_ce_gama=qkv_ce_gama, qkv_cross_gama=qkv_cross_gama, qkv_layout=qkv_layout, relation_layers=relation_layers)
        loss = out['loss']
        log_now = (step % print_freq == 0)
        if log_now:
            loss_value = loss.item()
            if not math.isfinite(loss_value):                                        # engine.py:119-121
                print("Loss is {}, stopping training".format(loss_value))
                sys.exit(1)
            metric_logger.update(cls_loss=out['cls_loss'].item(), q_loss=out['q_loss'].item(),
                                 k_loss=out['k_loss'].item(), v_loss=out['v_loss'].item(), loss=loss_value)
            for name in extra:
                metric_logger.update(**{name: out[name].item()})
        optimizer.zero_grad()
        loss_scaler(loss, optimizer, clip_grad=max_norm, parameters=model.parameters())
        if model_ema is not None:
            model_ema.update(model)
        if log_now:
            metric_logger.update(lr=optimizer.param_groups[0]["lr"])
        step += 1
    metric_logger.synchronize_between_processes()
    if log is not None:
        log.info(f"Averaged stats: {metric_logger}")
    return {k: meter.global_avg for k, meter in metric_logger.meters.items()}


def train_one_epoch(model, criterion, data_loader, optimizer, device, epoch, loss_scaler, log=None, max_norm=0,
                    model_ema=None, mixup_fn=None, print_freq=10):
    """train_subdata.py:233-286: the plain (teacher-in-criterion) training loop that produces the sub-dataset teachers
    and fine-tuned models -- `criterion` is losses.DistillationLoss(inputs, outputs, labels).  Same kernels as the DEKD
    step; `.item()` only every print_freq steps (the reference syncs every step, :266,:279)."""
    from .utils import MetricLogger, SmoothedValue
    model.train(True)
    metric_logger = MetricLogger(delimiter="  ")
    metric_logger.add_meter('lr', SmoothedValue(window_size=1, fmt='{value:.6f}'))
    header = 'Epoch: [{}]'.format(epoch)
    step = 0
    for samples, targets, _ in metric_logger.log_every(_PreparedBatches(data_loader, device, mixup_fn, None), print_freq, header):
        with de_vit.lean_tail(model):                                                # only the logits are read below
            outputs = model(samples)                                                 # :258
        loss = criterion(inputs=samples, outputs=outputs, labels=targets)            # :259
        if step % print_freq == 0:
            loss_value = loss.item()
            if not math.isfinite(loss_value):                                        # :263-265
                print("Loss is {}, stopping training".format(loss_value))
                sys.exit(1)
            metric_logger.update(loss=loss_value, lr=optimizer.param_groups[0]["lr"])
        optimizer.zero_grad()
        loss_scaler(loss, optimizer, clip_grad=max_norm, parameters=model.parameters())
        if model_ema is not None:
            model_ema.update(model)
        step += 1
    metric_logger.synchronize_between_processes()
    if log is not None:
        log.info(f"Averaged stats: {metric_logger}")
    return {k: meter.global_avg for k, meter in metric_logger.meters.items()}


@torch.no_grad()
def evaluate(data_loader, model, device):
    """engine.py:17-45: eval forward, CE, top-1 / top-5."""
    from .utils import MetricLogger, accuracy
    metric_logger = MetricLogger(delimiter="  ")
    model.eval()
    for images, target in metric_logger.log_every(data_loader, 10, 'Test:'):
        images = images.to(device, non_blocking=True)
        target = target.to(device, non_blocking=True)
        with de_vit.lean_tail(model):                                   # only the logits are read (engine.py:31-32)
            output = model(images)
        loss = losses.DistillLoss(losses.SoftTargetCrossEntropy(), 'none', 0., 1.)(output, None, target)
        acc1, acc5 = accuracy(output, target, topk=(1, min(5, output.shape[1])))
        metric_logger.update(loss=loss.item())
        metric_logger.meters['acc1'].update(acc1.item(), n=images.shape[0])
        metric_logger.meters['acc5'].update(acc5.item(), n=images.shape[0])
    metric_logger.synchronize_between_processes()
    return {k: meter.global_avg for k, meter in metric_logger.meters.items()}


# ------------------------------------------------------------------------------------------------------
# ensemble stage (engine.py:143-242): MultiViT backbones + EnsMLP fusion against the teacher
# ------------------------------------------------------------------------------------------------------
def ens_forward(model, ens_model, criterion, samples, targets, distillation_type="hard"):
    """engine.py:167-179: returns dict(loss, token_loss, cls_loss)."""
    features = model(samples)
    if distillation_type == 'none':
        logits = ens_model(features)
        loss = criterion(samples, logits, targets)
        return dict(loss=loss, token_loss=None, cls_loss=loss)
    outputs = ens_model(features, True)
    inter_loss, cls_loss = criterion(inputs=samples, stu_outputs=outputs, labels=targets)
    return dict(loss=inter_loss + cls_loss, token_loss=inter_loss, cls_loss=cls_loss)


def train_1epoch_ens_disjoint(model, ens_model, criterion, data_loader, optimizer, ens_optimizer, device, epoch, scaler,
                              args, log, model_ema=None, ens_model_ema=None, mixup_fn=None, max_norm=0, print_freq=10):
    """engine.py:143-210.  `optimizer` / `ens_optimizer` are any torch optimizers over the two parameter sets (the
    reference uses two AdamW instances); gradients arrive in param.grad.  `scaler` (the reference's loss scaler slot): None runs torch's tail
    -- coalesced gradient mean, clip_grad_norm_ per model, the two optimizers' step(); a runner `scaler(loss, optimizer, ens_optimizer,
    clip_grad=)` (ensemble.EnsStepRunner) does backward, the gradient exchange and both optimizer steps itself, on the flat fused path."""
    from .utils import MetricLogger, SmoothedValue
    model.train(True)
    ens_model.train(True)
    metric_logger = MetricLogger(delimiter="  ")
    for name in ('backbone_lr', 'ens_lr', 'cls_loss', 'token_loss'):
        metric_logger.add_meter(name, SmoothedValue(window_size=1, fmt='{value:.6f}'))
    step = 0
    for samples, targets in metric_logger.log_every(data_loader, print_freq, 'Epoch: [{}]'.format(epoch)):
        samples, targets = samples.to(device, non_blocking=True), targets.to(device, non_blocking=True)
        if mixup_fn is not None:
            samples, targets = mixup_fn(samples, targets)
        optimizer.zero_grad(set_to_none=True)
        ens_optimizer.zero_grad(set_to_none=True)
        out = ens_forward(model, ens_model, criterion, samples, targets, args.distillation_type)
        if scaler is not None:
            scaler(out['loss'], optimizer, ens_optimizer, clip_grad=max_norm)
        else:
            out['loss'].backward()
            # the gradient mean DistributedDataParallel produces for both wrapped models (ensemble.py:332-334); no-op at world 1
            from . import ddp
            ddp.allreduce_mean_([p.grad for p in model.parameters()] + [p.grad for p in ens_model.parameters()])
            if max_norm:
                torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm)
                torch.nn.utils.clip_grad_norm_(ens_model.parameters(), max_norm)
            optimizer.step()
            ens_optimizer.step()
        if step % print_freq == 0:
            lv = out['loss'].item()
            if not math.isfinite(lv):
                print(f"Loss is {lv}, stopping training")
                sys.exit(1)
            metric_logger.update(loss=lv, backbone_lr=optimizer.param_groups[0]["lr"], ens_lr=ens_optimizer.param_groups[0]["lr"])
            if out['token_loss'] is not None:
                metric_logger.update(token_loss=out['token_loss'].item(), cls_loss=out['cls_loss'].item())
        step += 1
    metric_logger.synchronize_between_processes()
    return {k: meter.global_avg for k, meter in metric_logger.meters.items()}


@torch.no_grad()
def evaluate_ens_disjoint(data_loader, model, ens_model, device):
    """engine.py:212-242: collaborative inference = N sub-model backbones + EnsMLP, CE, top-1 / top-5."""
    from .utils import MetricLogger, accuracy
    metric_logger = MetricLogger(delimiter="  ")
    model.eval()
    ens_model.eval()
    for images, target in metric_logger.log_every(data_loader, 10, 'Test:'):
        images, target = images.to(device, non_blocking=True), target.to(device, non_blocking=True)
        output = ens_model(model(images))
        loss = losses.DistillLoss(losses.SoftTargetCrossEntropy(), 'none', 0., 1.)(output, None, target)
        acc1, acc5 = accuracy(output, target, topk=(1, 5))
        metric_logger.update(loss=loss.item())
        metric_logger.meters['acc1'].update(acc1.item(), n=images.shape[0])
        metric_logger.meters['acc5'].update(acc5.item(), n=images.shape[0])
    metric_logger.synchronize_between_processes()
    return {k: meter.global_avg for k, meter in metric_logger.meters.items()}
