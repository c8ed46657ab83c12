"""Tensor-level wrappers over the C ABI (include/devit_hip.h) and the autograd Functions built on them.

PyTorch is plumbing here: it owns device memory and streams, autograd stitches the hand-written
forward/backward kernel sequences together.  Every GEMM, attention, LayerNorm, loss and optimizer kernel is behind the
C ABI; what torch itself still launches per step is glue -- a few dozen small elementwise kernels (zero-fills of fresh
buffers, combining the loss terms, the gradient adds autograd makes where two paths meet, scalar scales, the DropPath
mask draw: rand / floor / div) and ~25 runtime copies, about 0.3 ms of the 29.7 ms serialized step (measured as 0.33 ms
in profiles/r02_e_bench_serial_kernel_stats.csv, before the loss total moved onto the relation-loss vector).

Layout conventions
  * token rows: M = B * N; every bf16 activation that feeds a GEMM lives in a buffer whose row count is
    padded to a multiple of 128 with ZERO pad rows (`rows_alloc`): the GEMM tiles are 128 rows tall and
    the weight-gradient GEMMs reduce over the padded row count.
  * residual stream: fp32 [B, N, D]; branch activations / branch gradients: bf16.
  * the encoder blocks' launch sequence lives in C (csrc/encoder.hip: devit_encoder_fwd / devit_block_bwd, and devit_tail_fwd / devit_tail_bwd
    for the lean last block) and nowhere else; EncoderFn is those calls and the grouping of the weight gradients.  bench.py's instruments see
    the launches through the library's launch observer (`observing`), so the instrumented step is the step that runs.
  * weight gradients are ACCUMULATED straight into `param.grad` (fp32, allocated zero on first use), the
    way DDP "main_grad" fusions do; `backward` returns None for parameters and reports finished blocks
    through `grad_ready` callbacks (devit_amd/ddp.py hooks its bucket all-reduce there).
"""
import contextlib
import ctypes as C
import os

import numpy as np
import torch

from . import _lib as L
from ._lib import ptr, stream_ptr

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
ROW_TILE = 256


# ----------------------------------------------------------------------------------------------
# instruments: the library reports its launches (devit_set_launch_observer, include/devit_hip.h) to whoever observes this thread
# ----------------------------------------------------------------------------------------------
# bench.py's three instruments: each is None or a list, set by plain assignment and read back after the step.  While one is a list, every
# launch the library reports from a call made here is bracketed by events on the stream the kernels really go to:
PROFILE = None          # GEMM launches: (template, M, N, K, batch, start_event, end_event)
PROFILE_HBM = None      # the bandwidth-bound kernels (LayerNorm, attention): (name, algorithmic bytes, start_event, end_event)
PROFILE_WGRAD = None    # grouped weight-gradient launches: (algorithmic flops, algorithmic bytes, start_event, end_event)


def gemm_template(a_kmajor, b_kmajor, kind, fused_ln_bwd=False):
    """PROFILE's label of a GEMM launch.  The student's fc2 forward reads a k-major COPY of its weight on the full-row kernel (k-major B with the
    fp32 residual epilogue): still a forward Linear layer of the dominant template."""
    b_row = not b_kmajor or kind == L.EPI_RESIDUAL_F32
    return ("A_km" if a_kmajor else "A_row") + "/" + ("B_row" if b_row else "B_km") + ("+ln_bwd" if fused_ln_bwd else "")


def hbm_record(i):
    """(name, algorithmic bytes) of a reported LayerNorm / attention launch, None for anything else.  i: L.LaunchInfo."""
    def has(bit):
        return 1 if i.has & bit else 0
    name = i.name.decode()
    if name == "devit_layernorm_fwd":       # the fp32 rows in, the normalised rows out (bf16 and / or fp32)
        return "layernorm_fwd", i.rows * i.width * (4 + 2 * has(L.HAS_Y_BF16) + 4 * has(L.HAS_Y_F32))
    if name == "devit_layernorm_bwd":       # dy, x and the incoming residual gradient in; the fp32 gradient (and its bf16 copy) out
        return "layernorm_bwd", i.rows * i.width * ((4 if has(L.HAS_DY_F32) else 2) + 4 + 4 * has(L.HAS_DRES) + 4 * has(L.HAS_DX) +
                                                    2 * has(L.HAS_DX_BF16))
    if name == "devit_attn_fwd":            # q, k, v in, the head outputs out (bf16)
        return "attention_fwd", i.rows * i.width * 2 * 4
    if name == "devit_attn_bwd":            # q, k, v, o, do in; dq, dk, dv out (+ the relation-loss gradient that is added in)
        return "attention_bwd", i.rows * i.width * 2 * (8 + 3 * has(L.HAS_DQKV_ADD))
    if name == "devit_attn_fwd_rows":
        return "attention_fwd_rows", (i.rows * 2 * i.width + 2 * i.q_rows * i.width) * 2
    if name == "devit_attn_bwd_rows":
        return "attention_bwd_rows", (i.rows * 4 * i.width + 4 * i.q_rows * i.width) * 2
    return None


_observer = None        # the callback of the innermost observing() block
_observer_error = None


@L.LAUNCH_OBSERVER
def _on_launch(user, phase, stream, info):
    global _observer_error
    try:
        _observer(phase, stream, info.contents)
    except BaseException as e:       # (ctypes would print and swallow it: observing() re-raises it once the library call has returned)
        if _observer_error is None:
            _observer_error = e


@contextlib.contextmanager
def observing(callback):
    """Inside the block, callback(phase, stream, info) runs for every launch the library reports from THIS thread: phase 0 just before the entry
    point's first kernel, 1 just after its last; stream: the hipStream_t (int or None) the kernels go to; info: L.LaunchInfo, valid during the
    callback only.  An exception raised by the callback leaves the block once the library call it interrupted has returned."""
    global _observer, _observer_error
    prev, _observer = _observer, callback
    L.call("devit_set_launch_observer", _on_launch, None)
    try:
        yield
    finally:
        _observer = prev
        if prev is None:
            L.call("devit_set_launch_observer", L.LAUNCH_OBSERVER(0), None)
        err, _observer_error = _observer_error, None
    if err is not None:
        raise err


def torch_stream(stream):
    """The hipStream_t a launch was reported on, as the torch stream to record events on.  torch's own object where it is the current stream: an
    ExternalStream made from the default stream's handle (0) does not bracket the kernels -- measured: 6-15 us around every launch, some negative."""
    cur = torch.cuda.current_stream()
    return cur if cur.cuda_stream == (stream or 0) else torch.cuda.ExternalStream(stream)


_start = None           # the start event of the launch being reported (reports do not nest)


def _record(phase, stream, i):
    """The observer behind PROFILE / PROFILE_HBM / PROFILE_WGRAD: events on the stream the launch goes to, not on the current one."""
    global _start
    name = i.name.decode()
    rec = PROFILE_WGRAD if name == "devit_wgrad_grouped" else PROFILE if name in ("devit_gemm_bf16", "devit_dgrad_layernorm_bwd") else PROFILE_HBM
    if rec is None:
        return
    ev = torch.cuda.Event(enable_timing=True)
    ev.record(torch_stream(stream))
    if phase == 0:
        _start = ev
    elif name == "devit_wgrad_grouped":
        rec.append((i.flops, i.bytes, _start, ev))
    elif rec is PROFILE:
        rec.append((gemm_template(i.a_kmajor, i.b_kmajor, i.kind, name == "devit_dgrad_layernorm_bwd"), i.M, i.N, i.K, i.batch, _start, ev))
    else:
        rec.append(hbm_record(i) + (_start, ev))


# ----------------------------------------------------------------------------------------------
# deterministic mode (include/devit_hip.h, "Deterministic mode"): fixed-order reductions instead of fp32 atomics in arrival order
# ----------------------------------------------------------------------------------------------
_det_ws = {}            # device index -> the registered workspace (kept alive here; allocated once, at the first launch in the mode)


def is_deterministic():
    on = bool(L.load().devit_get_deterministic())
    L.before_call = _det_workspace if on else None
    return on


def set_deterministic(flag):
    """Process-wide, off by default.  On: every reduction of the training step that combines partial sums by fp32 atomics runs in a fixed order
    instead (same input, seed and launch configuration -> same bits, at world size 1).  Needs no device."""
    L.before_call = None
    L.call("devit_set_deterministic", int(bool(flag)))
    is_deterministic()


@contextlib.contextmanager
def deterministic(flag=True):
    """`with ops.deterministic():` -- the mode inside the block, the previous state behind it (also when the block raises)."""
    prev = is_deterministic()
    set_deterministic(flag)
    try:
        yield
    finally:
        set_deterministic(prev)


def _det_workspace():
    """Register the current device's workspace with the library, once: L.before_call while the mode is on, so every entry point finds it."""
    if not torch.cuda.is_available():
        return
    dev = torch.cuda.current_device()
    if dev not in _det_ws:
        ws = _det_ws[dev] = torch.empty(int(L.load().devit_det_workspace_bytes()), dtype=torch.uint8, device=torch.device("cuda", dev))
        L.call("devit_set_det_workspace", ptr(ws), ws.numel())


def _det_first_call():
    """The library's default comes from DEVIT_DETERMINISTIC: asked at the first call, when the library is there to be asked."""
    if is_deterministic():
        _det_workspace()


L.before_call = _det_first_call


def call(name, *args):
    """_lib.call; while an instrument is set, with its observer around the call."""
    if (PROFILE is None and PROFILE_HBM is None and PROFILE_WGRAD is None) or _observer is not None:
        return L.call(name, *args)
    with observing(_record):
        return L.call(name, *args)


def pad_rows(m):
    return (m + ROW_TILE - 1) // ROW_TILE * ROW_TILE


def qkv_pad_rows(N):
    """Zeroed rows behind a packed qkv buffer that the relation loss reads (csrc/encoder.hip: qkv_pad_rows; DEVIT_BLK_QKV_PAD): its Gram
    windows are 256 rows per image, so the last image needs 256 - N rows behind its own -- inside the usual 128 from N = 128 on."""
    return 128 if N >= 128 else 256 - N


def rows_alloc(m, cols, dtype, device, extra=0):
    """[pad_rows(m) + extra, cols] buffer whose rows >= m are zero."""
    mp = pad_rows(m) + extra
    t = torch.empty((mp, cols), dtype=dtype, device=device)
    if mp > m:
        t[m:].zero_()
    return t


_ws_cache = {}


def workspace(device, nbytes):
    key = (device.index, torch.cuda.current_stream().cuda_stream)
    t = _ws_cache.get(key)
    if t is None or t.numel() < nbytes:
        t = torch.empty(max(nbytes, 8 << 20), dtype=torch.uint8, device=device)
        _ws_cache[key] = t
    return t


# ----------------------------------------------------------------------------------------------
# thin wrappers
# ----------------------------------------------------------------------------------------------
def gemm(a, lda, a_km, b, ldb, b_km, M, N, K, *, kind, out, ldc, bias=None, colscale=None, aux=None, aux_in=None,
         res=None, rowscale=None, rows_per_scale=0, pos=None, patch_tokens=0, extra_tokens=0, exact_gelu=0, batch=1,
         a_bs=0, b_bs=0, out_bs=0, m_valid=0, split_k=1, a_group=0, a_skip=0, b_group=0, b_skip=0, dtype16=0):
    A = L.Operand(a.data_ptr(), lda, a_km, a_group, a_skip, a_bs)
    Bo = L.Operand(b.data_ptr(), ldb, b_km, b_group, b_skip, b_bs)
    ep = L.Epilogue(kind, out.data_ptr(), ldc, _p(bias), _p(colscale), _p(aux), _p(aux_in), _p(res), _p(rowscale),
                    rows_per_scale, _p(pos), patch_tokens, extra_tokens, exact_gelu, out_bs, m_valid, dtype16)
    call("devit_gemm_bf16", C.byref(A), C.byref(Bo), M, N, K, batch, split_k, C.byref(ep), stream_ptr())


def _p(t):
    return None if t is None else t.data_ptr()


def gemm_route(a, lda, a_km, b, ldb, b_km, M, N, K, *, kind, out, ldc, bias=None, colscale=None, aux=None, aux_in=None,
               res=None, rowscale=None, rows_per_scale=0, pos=None, patch_tokens=0, extra_tokens=0, exact_gelu=0, batch=1,
               a_bs=0, b_bs=0, out_bs=0, m_valid=0, split_k=1, a_group=0, a_skip=0, b_group=0, b_skip=0, dtype16=0):
    """devit_gemm_route() itself for the arguments gemm() takes (csrc/gemm.hip; no GPU needed, tensors of any device or plain integer addresses):
    the L.ROUTE_* kernel the call would run on, or the negative DEVIT_ERR_* its argument checks return.  Not a restatement: one rule."""
    def adr(t):
        return t if t is None or isinstance(t, int) else t.data_ptr()
    if L.before_call is not None:         # (deterministic mode: the query sees the workspace the launch would find)
        L.before_call()
    A = L.Operand(adr(a), lda, a_km, a_group, a_skip, a_bs)
    Bo = L.Operand(adr(b), ldb, b_km, b_group, b_skip, b_bs)
    ep = L.Epilogue(kind, adr(out), ldc, adr(bias), adr(colscale), adr(aux), adr(aux_in), adr(res), adr(rowscale),
                    rows_per_scale, adr(pos), patch_tokens, extra_tokens, exact_gelu, out_bs, m_valid, dtype16)
    return int(L.load().devit_gemm_route(C.byref(A), C.byref(Bo), M, N, K, batch, split_k, C.byref(ep)))


def full_row_selected(M, N, K, kind=L.EPI_RESIDUAL_F32):
    """devit_gemm_full_row_selected() itself (csrc/gemm.hip; no GPU needed): would (row-major A) x (K-MAJOR B) with N outputs run on the full-row
    256x384 kernel?  (A k-major weight with the fp32 residual epilogue exists on that kernel only.)  Not a restatement: one rule, one parser of
    DEVIT_GEMMFR."""
    return bool(L.load().devit_gemm_full_row_selected(M, N, K, kind))


# Anything that rewrites 16-bit weight copies IN PLACE (behind the parameters' version counters: the fused optimizer kernel, FlatParams.refresh_bf16)
# re-transposes the k-major copies that were derived from them (transpose16_jobs below); copies re-made by de_vit._w16 are re-derived there.
def transpose16(src, dst):
    """dst[c][r] = src[r][c] for 16-bit matrices (devit_index_copy mode 4): the k-major copy of a Linear weight."""
    _Transposes([(src, dst)]).run()


class _Transposes:
    """A device-resident devit_index_job table of 16-bit transposes, one launch."""

    def __init__(self, pairs):
        jobs = [L.IndexJob(s_.data_ptr(), d.data_ptr(), None, s_.shape[0], s_.shape[1], s_.stride(0), d.stride(0), 4, 2) for s_, d in pairs]
        arr = (L.IndexJob * len(jobs))(*jobs)
        self.table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(pairs[0][0].device)
        self.keep, self.n = pairs, len(jobs)
        self.key = tuple((s_.data_ptr(), d.data_ptr()) for s_, d in pairs)
        self.blocks = max(1, min(144, max((s_.shape[0] + 63) // 64 * ((s_.shape[1] + 63) // 64) for s_, _ in pairs)))   # one 64 x 64 tile per block

    def run(self):
        call("devit_index_copy", ptr(self.table), self.n, self.blocks, stream_ptr())


def split_k_for(out_rows, out_cols, ksteps):
    """Split-K factor of a weight-gradient GEMM: exactly one round of resident workgroups (128x128 tiles, two per
    CU).  More slices only add fp32-atomic traffic (64 KB per workgroup at ~1.3 TB/s chip-wide): measured 640 vs 521
    TFLOP/s (fc1, 14 vs 28 slices), 590 vs 460 (qkv, 18 vs 37)."""
    tiles = (out_rows // 128) * (out_cols // 128)     # wgrad always runs 128x128 tiles, two workgroups per CU
    slots = 512
    return max(1, min(ksteps, slots // tiles))


def linear_fwd(x, w, bias, M, *, out, kind=L.EPI_STORE_BF16, **kw):
    """out[M, N] = x[Mp, K] @ w[N, K]^T (+ epilogue).  x is a padded bf16 buffer."""
    N, K = w.shape
    gemm(x, x.stride(0), 0, w, K, 0, pad_rows(M), N, K, kind=kind, out=out, ldc=out.stride(0), bias=bias, m_valid=M,
         **kw)


def linear_dgrad(dy, w, M, *, out, kind=L.EPI_STORE_BF16, **kw):
    """out[M, K] = dy[Mp, N] @ w[N, K]   (w read k-major)."""
    N, K = w.shape
    gemm(dy, dy.stride(0), 0, w, K, 1, pad_rows(M), K, N, kind=kind, out=out, ldc=out.stride(0), m_valid=M, **kw)


def linear_wgrad(dy, x, w_grad, b_grad, M, **kw):
    """w_grad[N, K] += dy[Mp, N]^T @ x[Mp, K];  b_grad[N] += colsum(dy), one launch.  Pad rows of dy are zero."""
    N, K = w_grad.shape
    mp = pad_rows(M)
    # b_grad: the row sums of dy^T come out of the same launch (fragments the MFMAs read anyway; no second pass over dy)
    gemm(dy, dy.stride(0), 1, x, x.stride(0), 1, N, K, mp, kind=L.EPI_ATOMIC_F32, out=w_grad, ldc=K,
         split_k=split_k_for(N, K, mp // 64), aux=b_grad, **kw)


def wgrad_jobs_ok(mp, jobs):
    """Can these weight gradients run as ONE launch of the full-row weight-gradient kernel (devit_wgrad_grouped)?  jobs: (dy, x, w_grad, b_grad)
    as linear_wgrad takes them.  One side of every product must be exactly 384 features wide (the student's D), the other a multiple of 128
    (wgrad_job_struct says which); DEVIT_WGRADFR=0 keeps the split-K launches on 128x128 tiles."""
    return wgrad_enabled(mp) and len(jobs) <= L.WGRAD_MAX_JOBS and all(
        (w.shape[1] == 384 and w.shape[0] % 128 == 0) or (w.shape[0] == 384 and w.shape[1] % 128 == 0) for _, _, w, _ in jobs)


def linear_wgrads(jobs, M, split_k=0):
    """The weight (and bias) gradients of several Linear layers in ONE launch: jobs = [(dy [Mp, N], x [Mp, K], w_grad [N, K], b_grad [N] or None)].
    w_grad += dy^T x; b_grad += colsum(dy).  K == 384: tiles over dy's features; N == 384 (fc2): the product is taken transposed (tiles over x's
    features) and its bias gradient, if asked for, comes from a column-sum pass."""
    mp = pad_rows(M)
    structs, late = [], []
    for dy, x, w_grad, b_grad in jobs:
        if w_grad.shape[1] != 384 and b_grad is not None:     # (the transposed product has no bias-gradient side: a column-sum pass behind the launch)
            late.append((dy, b_grad))
            b_grad = None
        j = wgrad_job_struct(dy, x, w_grad, b_grad)
        if j is None:
            raise L.DevitError(f"linear_wgrads: a {tuple(w_grad.shape)} weight gradient does not fit the full-row kernel (wgrad_jobs_ok)")
        structs.append(j)
    arr = (L.WgradJob * len(jobs))(*structs)
    call("devit_wgrad_grouped", arr, len(jobs), mp, split_k, stream_ptr())
    for dy, b_grad in late:
        colsum(dy, mp, b_grad.shape[0], b_grad, True)


def wgrad_enabled(mp):
    """DEVIT_WGRADFR=0 keeps every weight gradient on the split-K 128x128 launches (read per call, as devit_block_bwd reads it)."""
    e = os.environ.get("DEVIT_WGRADFR", "")
    return (e == "" or int(e) != 0) and mp % 64 == 0 and mp // 64 >= 3


def colsum(y, M, N, out, accumulate, row_group=0, row_skip=0):
    nbytes = 64 * N * 4
    ws = workspace(y.device, nbytes)
    call("devit_colsum_bf16", ptr(y), M, N, y.stride(0), row_group, row_skip, ptr(out), int(accumulate), ptr(ws),
         ws.numel(), stream_ptr())


def layernorm_fwd(x2d, rows, D, gamma, beta, eps, *, y_bf16=None, y_f32=None, mean=None, rstd=None, in_group=0,
                  in_stride=0, dtype16=0):
    call("devit_layernorm_fwd", ptr(x2d), rows, D, in_group, in_stride, ptr(gamma), ptr(beta), eps, ptr(y_bf16),
         ptr(y_f32), ptr(mean), ptr(rstd), dtype16, stream_ptr())


def layernorm_bwd(dy, dy_is_f32, x2d, rows, D, mean, rstd, gamma, dres, dx, dx_bf16, rowscale, rows_per_scale, dgamma,
                  dbeta, in_group=0, in_stride=0, gsum=None):
    ws = workspace(x2d.device, L.load().devit_layernorm_bwd_workspace(rows, D))
    call("devit_layernorm_bwd", ptr(dy), int(dy_is_f32), ptr(x2d), rows, D, in_group, in_stride, ptr(mean), ptr(rstd),
         ptr(gamma), ptr(dres), ptr(dx), ptr(dx_bf16), ptr(rowscale), rows_per_scale, ptr(dgamma), ptr(dbeta),
         ptr(gsum), 1, ptr(ws), ws.numel(), stream_ptr())


def cast_bf16(src, dst=None, f16=False):
    """fp32 -> bf16 (or IEEE f16: the frozen teacher's GEMM weights) copy of a tensor."""
    src = src.contiguous()
    if dst is None:
        dst = torch.empty(src.shape, dtype=F16 if f16 else BF16, device=src.device)
    call("devit_cast_bf16", ptr(src), ptr(dst), src.numel(), int(dst.dtype == F16), stream_ptr())
    return dst


_ONES1 = {}


def _ones1(dev):
    """A cached fp32 [1.0] on `dev` (the ones-vector operand of the bias-gradient sgemm calls)."""
    t = _ONES1.get(dev)
    if t is None:
        t = _ONES1[dev] = torch.ones(1, dtype=F32, device=dev)
    return t


class GradSlot:
    """Stands where a parameter stands in BlockParams when the block runs on COMPACTED weights (shrink.compact): the
    weight-gradient GEMMs accumulate into `.grad` [compact shape] and BlockParams.finish_grads() adds it into the kept
    rows / columns of the fp32 master's gradient."""
    __slots__ = ("shape", "device", "grad", "requires_grad")

    def __init__(self, shape, device):
        self.shape, self.device, self.grad, self.requires_grad = tuple(shape), device, None, False


def grad_buf(p):
    """fp32 accumulation buffer of a parameter (== param.grad, zero-initialised on first use)."""
    p = getattr(p, "slot", p)             # a compact bias: the value the kernels read + the slot its gradient goes to
    if p.grad is None:
        if isinstance(p, GradSlot):
            p.grad = torch.zeros(p.shape, dtype=F32, device=p.device)
        else:
            p.grad = torch.zeros_like(p, memory_format=torch.contiguous_format)
    return p.grad


def sgemm_small(A, sam, sak, Bm, sbn, sbk, bias, Cm, ldc, M, N, K, alpha=1.0, accumulate=False):
    call("devit_sgemm_small", ptr(A), sam, sak, ptr(Bm), sbn, sbk, ptr(bias), ptr(Cm), ldc, M, N, K, alpha,
         int(accumulate), stream_ptr())


class DeferredWgrads:
    """The weight gradients of SEVERAL blocks in one launch of the full-row weight-gradient kernel (devit_wgrad_grouped).  A block's four
    products are 19 tiles of 256 x 384: alone they need 13 K slices to fill 256 CUs, and the slices' fp32 atomics (97 MB per block at the
    ~1.3 TB/s the memory side adds floats at) are a third of the launch.  Grouped over g blocks the same CUs are filled by 13 / g slices:
    the blocks' backward records its products as jobs (devit_block_bwd_io.defer_jobs) and the group is launched
    -- and its blocks reported to `grad_ready` -- behind the backward of its last block.  Groups (DEVIT_WGRAD_GROUP=auto|all|block):
      auto   with a gradient exchange to overlap (a reducer with world > 1 on `grad_ready`): the blocks of one reducer bucket, so that every
             bucket still leaves as soon as its gradients exist; without one: all blocks of the encoder call (one launch, no K split)
      all    one group        bucket  the reducer's buckets whatever the world size        block  every block alone (round 6's first form)"""

    def __init__(self, cfg, nb):
        self.cfg, self.jobs, self.pending, self.keep = cfg, [], [], []
        hook = cfg.grad_ready
        policy = os.environ.get("DEVIT_WGRAD_GROUP", "auto")
        if policy not in ("auto", "all", "block", "bucket"):
            raise L.DevitError(f"DEVIT_WGRAD_GROUP={policy!r}: auto, all, bucket or block")
        has_buckets = getattr(hook, "bucket_of", None) is not None
        if policy == "auto":
            policy = "bucket" if (has_buckets and getattr(hook, "world", 1) > 1) else "all"
        elif policy == "bucket" and not has_buckets:      # (no reducer on this model: nothing to align with)
            policy = "all"
        self.policy = policy
        self.bucket = [hook.bucket_of(bp.all_params()) for bp in cfg.blocks[:nb]] if policy == "bucket" else None

    def last_of_group(self, i):
        """Is block i the last (lowest) block of its group?  (backward walks i downwards)"""
        if i == 0 or self.policy == "block" or len(self.jobs) + 4 > L.WGRAD_MAX_JOBS:   # (no room for the next block's four)
            return True
        return self.policy == "bucket" and self.bucket[i] != self.bucket[i - 1]

    def add(self, bp, jobs, keep=()):
        """jobs: L.WgradJob structs of block bp, whose backward has just been enqueued; keep: whatever owns the memory they point into"""
        self.jobs += jobs
        self.pending.append(bp)
        self.keep.extend(keep)

    def flush(self, mp):
        if self.jobs:
            arr = (L.WgradJob * len(self.jobs))(*self.jobs)
            call("devit_wgrad_grouped", arr, len(self.jobs), mp, 0, stream_ptr())
        for bp in self.pending:
            bp.finish_grads()
            if self.cfg.grad_ready is not None:
                self.cfg.grad_ready(bp.all_params())
        self.jobs, self.pending, self.keep = [], [], []


def wgrad_job_struct(dy, x, w_grad, b_grad):
    """One product of linear_wgrads() as a devit_wgrad_job (None if the full-row weight-gradient kernel does not take it)."""
    N, K = w_grad.shape
    j = L.WgradJob()
    if K == 384 and N % 128 == 0:
        j.a, j.lda, j.a_cols, j.b, j.ldb = dy.data_ptr(), dy.stride(0), N, x.data_ptr(), x.stride(0)
        j.out, j.ldc, j.transposed, j.a_colsum = w_grad.data_ptr(), K, 0, _p(b_grad)
        return j
    if N == 384 and K % 128 == 0 and b_grad is None:
        j.a, j.lda, j.a_cols, j.b, j.ldb = x.data_ptr(), x.stride(0), K, dy.data_ptr(), dy.stride(0)
        j.out, j.ldc, j.transposed, j.a_colsum = w_grad.data_ptr(), K, 1, None
        return j
    return None


# ----------------------------------------------------------------------------------------------
# encoder blocks (models/de_vit.py:103-121 x depth) as ONE autograd node
# ----------------------------------------------------------------------------------------------
class BlockParams:
    """fp32 parameters + cached bf16 GEMM copies of one Block (see de_vit.Block)."""
    __slots__ = ("n1w", "n1b", "qkv_w", "qkv_b", "proj_w", "proj_b", "n2w", "n2b", "fc1_w", "fc1_b", "fc2_w", "fc2_b",
                 "qkv_w16", "proj_w16", "fc1_w16", "fc2_w16", "fc2_w16t", "num_heads", "head_gate", "neuron_gate", "dp_prob",
                 "module", "compacted", "masters", "finish")

    def all_params(self):
        """The nn.Parameters behind this block (the masters when the block runs compacted)."""
        if getattr(self, "masters", None) is not None:
            return self.masters
        return [self.n1w, self.n1b, self.qkv_w, self.qkv_b, self.proj_w, self.proj_b, self.n2w, self.n2b, self.fc1_w,
                self.fc1_b, self.fc2_w, self.fc2_b]

    def finish_grads(self):
        """After the block's backward: compacted blocks add their compact weight gradients into the masters'."""
        f = getattr(self, "finish", None)
        if f is not None:
            f()


class EncoderCfg:
    """Non-tensor arguments of EncoderFn."""

    def __init__(self, blocks, training, dp_scales, want_qkv, want_att, want_enc, eps=1e-6, exact_gelu=0,
                 grad_ready=None, qkv_pad_layers=None, lean_tokens=0, enc_layers=None):
        self.blocks, self.training, self.dp_scales = blocks, training, dp_scales
        # with want_enc: the blocks whose output is handed out in the 'encoder' list (None: every block); the others come back as None
        self.enc_layers = None if enc_layers is None else frozenset(enc_layers)
        self.want_qkv, self.want_att, self.want_enc = want_qkv, want_att, want_enc
        self.eps, self.exact_gelu, self.grad_ready = eps, exact_gelu, grad_ready
        # blocks whose packed qkv output gets the zeroed overhang rows RelationLossFn reads (None: every block)
        self.qkv_pad_layers = qkv_pad_layers
        # > 0: the caller reads only the first `lean_tokens` rows of every image of the encoder output (the class /
        # distillation tokens, models/de_vit.py:286-288) and nothing of the last block besides: that block then runs on its token rows
        # (devit_tail_fwd / devit_tail_bwd) and the output is [B, lean_tokens, D]
        self.lean_tokens = lean_tokens
        # dropout p > 0 of a TRAINING forward: None, or (seed, [(p, p_attn) per block]) -- the masks are functions of the seed (dropout.py), so
        # this is all a backward needs to regenerate them
        self.drop = None


# ----------------------------------------------------------------------------------------------
# whole blocks per ctypes call (devit_encoder_fwd / devit_block_bwd, devit_tail_fwd / devit_tail_bwd; csrc/encoder.hip): the ONE host sequence
# of the 16-bit block -- there is no restatement of it here.  One arena per block of an encoder call holds its activations; the instruments above see its
# launches through the library's observer.
# ----------------------------------------------------------------------------------------------
# Stream whose allocator pool the encoder arenas come from (None: the current stream).  A forward that runs on a side
# stream but is consumed on the main stream (the frozen teacher, engine._teacher_forward_async) sets this to the
# CONSUMER's stream: a 13 GB arena handed across streams with Tensor.record_stream() comes back to the allocator only when
# the recorded event has completed, i.e. a step later -- the host, which runs ahead, would hipMalloc a fresh arena every
# step (measured: 180 ms of host time per step).  With the arena in the consumer's pool the hand-over is ordered by the
# wait_stream() calls that are there anyway (producer starts after the consumer stream's tail, consumer joins the producer).
ARENA_ALLOC_STREAM = None
_sizes_cache = {}


def _arena(nbytes, dev):
    if ARENA_ALLOC_STREAM is not None and dev.type == "cuda":
        with torch.cuda.stream(ARENA_ALLOC_STREAM):
            return torch.empty(nbytes, dtype=torch.uint8, device=dev)
    return torch.empty(nbytes, dtype=torch.uint8, device=dev)
_ACT_DT = {L.ACT_LN1: BF16, L.ACT_QKV: BF16, L.ACT_ATTN_O: BF16, L.ACT_ATT: BF16, L.ACT_LN2: BF16, L.ACT_H: BF16,
           L.ACT_H_PRE: BF16}


def _sizes(name, count, *args):
    """One of the library's sizes functions -> (sizes, their byte offsets in one allocation, total), cached."""
    key = (name,) + args
    v = _sizes_cache.get(key)
    if v is None:
        sz = (C.c_size_t * count)()
        call(name, *args, sz)
        offs, off = [], 0
        for n in sz:
            offs.append(off)
            off += n
        v = _sizes_cache[key] = (list(sz), offs, off)
    return v


def _act_sizes(B, N, D, Da, Hd, flags):
    return _sizes("devit_block_acts_sizes", L.ACT_COUNT, B, N, D, Da, Hd, flags)


def _bwd_sizes(B, N, D, widths):
    """Transient buffers of devit_block_bwd, sized for the widest of `widths` = {(attn_width, hidden)} (compacted blocks of one
    model differ)."""
    key = ("b", B, N, D, tuple(sorted(widths)))
    v = _sizes_cache.get(key)
    if v is None:
        mx = [0] * L.BWD_COUNT
        for Da, Hd in widths:
            sz = (C.c_size_t * L.BWD_COUNT)()
            call("devit_block_bwd_sizes", B, N, D, Da, Hd, sz)
            mx = [max(a, b) for a, b in zip(mx, sz)]
        offs, off = [], 0
        for n in mx:
            offs.append(off)
            off += n
        v = _sizes_cache[key] = (mx, offs, off)
    return v


def _weights_struct(bp):
    w = L.BlockWeights()
    w.n1w, w.n1b, w.qkv_b, w.proj_b = bp.n1w.data_ptr(), bp.n1b.data_ptr(), bp.qkv_b.data_ptr(), bp.proj_b.data_ptr()
    w.n2w, w.n2b, w.fc1_b, w.fc2_b = bp.n2w.data_ptr(), bp.n2b.data_ptr(), bp.fc1_b.data_ptr(), bp.fc2_b.data_ptr()
    w.qkv_w16, w.proj_w16 = bp.qkv_w16.data_ptr(), bp.proj_w16.data_ptr()
    w.fc1_w16, w.fc2_w16 = bp.fc1_w16.data_ptr(), bp.fc2_w16.data_ptr()
    w.head_gate, w.neuron_gate = _p(bp.head_gate), _p(bp.neuron_gate)
    w.num_heads, w.attn_width, w.hidden = bp.num_heads, bp.qkv_w16.shape[0] // 3, bp.fc1_w16.shape[0]
    w.dtype16 = 1 if bp.qkv_w16.dtype == F16 else 0
    w.fc2_w16t = _p(getattr(bp, "fc2_w16t", None))
    return w


class _EncoderRun:
    """What one composite forward leaves behind for backward: the ctypes argument arrays and the arena they point into."""
    __slots__ = ("weights", "acts", "arena", "x", "dims", "views", "dps", "nb", "drops", "drop_tmp")


def _encoder_forward_composite(x, cfg, need_grad, nb):
    """Blocks [0, nb) of cfg.blocks."""
    B, N, D = x.shape
    M, dev = B * N, x.device
    mp = pad_rows(M)
    weights = (L.BlockWeights * nb)()
    acts = (L.BlockActs * nb)()
    run = _EncoderRun()
    # one allocation per block (uniform sizes: the caching allocator hands the same blocks back every step; a single
    # 8-13 GB arena per encoder call gets split by other requests and re-hipMalloc'ed -- measured 150 ms of host per step)
    run.weights, run.acts, run.arena, run.x, run.dims, run.dps, run.nb = weights, acts, [], x, (B, N, D), cfg.dp_scales, nb
    views = []
    x_ptr = x.data_ptr()
    for i, bp in enumerate(cfg.blocks[:nb]):
        weights[i] = _weights_struct(bp)
        pad = bool(cfg.want_qkv) and (cfg.qkv_pad_layers is None or i in cfg.qkv_pad_layers)
        flags = (L.BLK_SAVE if need_grad else 0) | (L.BLK_QKV_PAD if pad else 0) | (L.BLK_ATT if cfg.want_att else 0)
        Da, Hd = weights[i].attn_width, weights[i].hidden
        dt = F16 if weights[i].dtype16 else BF16
        if weights[i].dtype16 and need_grad:
            raise L.DevitError('precision="f16" is forward-only (frozen teacher): run it under torch.no_grad()')
        sz, offs, tot = _act_sizes(B, N, D, Da, Hd, flags)
        arena = _arena(tot, dev)
        run.arena.append(arena)
        base = arena.data_ptr()
        a = acts[i]
        a.x = x_ptr
        for j in range(L.ACT_COUNT):
            a.buf[j] = base + offs[j] if sz[j] else None
        dp = cfg.dp_scales[i] if cfg.dp_scales is not None else None
        a.dp1, a.dp2 = (_p(dp[0]), _p(dp[1])) if dp is not None else (None, None)
        a.flags = flags
        x_ptr = a.buf[L.ACT_X2]

        def view(j, rows, cols, dt, arena=arena, offs=offs):
            return arena[offs[j]:offs[j] + rows * cols * dt.itemsize].view(dt).view(rows, cols)
        qkv_rows = mp + (qkv_pad_rows(N) if flags & L.BLK_QKV_PAD else 0)
        v = dict(qkv=view(L.ACT_QKV, qkv_rows, 3 * Da, dt), x2=view(L.ACT_X2, M, D, F32).view(B, N, D),
                 att=view(L.ACT_ATT, M, D, dt) if cfg.want_att else None)
        v["qkv"]._devit_arena = True          # a view of an arena from ARENA_ALLOC_STREAM's pool (engine._hand_over)
        views.append(v)
        if bp.module is not None and not cfg.lean_tokens:  # shrink contract (core/imp_rank.py:31,108): post-mask values
            bp.module.mlp.neuron_output = view(L.ACT_H, mp, Hd, dt)[:M].view(B, N, Hd)
            bp.module.attn.head_output = view(L.ACT_ATTN_O, mp, Da, dt)[:M].view(B, N, bp.num_heads, Da // bp.num_heads)
        elif bp.module is not None:
            # inside de_vit.lean_tail the caller has declared that it reads the logits (and the middle block's q / k / v) only: the
            # debug views are not handed out, and the ones an earlier public forward left are dropped, so a ranking pass run inside
            # lean_tail fails loudly instead of reading stale values.  (This does NOT shrink the 35 GB peak: the per-layer q / k / v
            # views of the returned dict hold the arenas too, and those must stay until the consumer stream has read them -- the
            # arenas of a side-stream forward live in the CONSUMER's pool (ARENA_ALLOC_STREAM); dropping the unread layers' views
            # at once hands their memory to the main stream while the teacher's kernels still write it: measured as a non-finite
            # loss in the two-stream bench, round 4.)
            bp.module.mlp.neuron_output = None
            bp.module.attn.head_output = None
    run.views = views
    run.drops = run.drop_tmp = None
    if cfg.drop is not None:         # p > 0: the same sequence with the dropout passes in it (csrc/encoder.hip); p == 0 never comes here
        if cfg.want_att:
            raise L.DevitError("output_att under dropout p > 0 is not taken on the 16-bit path: run the model with precision=\"f32\"")
        run.drops, run.drop_tmp = _drop_structs(cfg.drop, nb, mp, D, dev)
        call("devit_encoder_fwd_drop", nb, weights, acts, run.drops, B, N, D, cfg.eps, stream_ptr())
        return run
    call("devit_encoder_fwd", nb, weights, acts, B, N, D, cfg.eps, stream_ptr())
    return run


def _drop_structs(drop, nb, mp, D, dev):
    """(L.BlockDropout * nb, the fp32 temporary they share) of EncoderCfg.drop"""
    from . import dropout
    seed, rates = drop
    tmp = torch.empty((mp, D), dtype=F32, device=dev)
    arr = (L.BlockDropout * nb)()
    for i in range(nb):
        (thr, s), (thr_a, s_a) = dropout.threshold(rates[i][0]), dropout.threshold(rates[i][1])
        arr[i].seed, arr[i].block, arr[i].thr, arr[i].thr_attn = seed, i, thr, thr_a
        arr[i].scale_keep, arr[i].scale_keep_attn, arr[i].tmp = s, s_a, tmp.data_ptr()
    return arr, tmp


def _wgrads_struct(bp):
    g = L.BlockWgrads()
    g.n1w, g.n1b, g.qkv_w, g.qkv_b = (grad_buf(p).data_ptr() for p in (bp.n1w, bp.n1b, bp.qkv_w, bp.qkv_b))
    g.proj_w, g.proj_b, g.n2w, g.n2b = (grad_buf(p).data_ptr() for p in (bp.proj_w, bp.proj_b, bp.n2w, bp.n2b))
    g.fc1_w, g.fc1_b, g.fc2_w, g.fc2_b = (grad_buf(p).data_ptr() for p in (bp.fc1_w, bp.fc1_b, bp.fc2_w, bp.fc2_b))
    return g


def _encoder_backward_composite(run, cfg, dx, dqkvs, defer, dencs=None):
    """dx: fp32 [B,N,D] contiguous gradient of the encoder output.  Returns the gradient of the encoder input.
    dencs: None, or per block of the run the fp32 [B,N,D] gradient that arrived for its exposed output (None where none did): added to the
    residual-stream gradient before that block's backward runs (ops_f32.EncoderF32Fn.backward).  The top block's is added to dx here; block
    i < nb - 1 gets its through devit_add_scale_cast_bf16 between the calls for blocks i + 1 and i: dx_in += denc_i, and the bf16 branch
    gradient g of block i, which block i + 1's LayerNorm backward wrote from the old dx_in, is rewritten as bf16(dp2_i * dx_in) -- one rounding of
    the sum.  Block i + 1 then hands down no fc2 bias gradient (it would be the column sums of the stale g): block i takes its own."""
    B, N, D = run.dims
    M, dev, nb = B * N, dx.device, run.nb
    if dencs is not None and not any(d is not None for d in dencs):
        dencs = None
    if dencs is not None:
        for d in dencs:
            if d is not None and (tuple(d.shape) != (B, N, D) or d.dtype != F32):
                raise L.DevitError(f"EncoderFn.backward: the gradient of an 'encoder' output must be fp32 {(B, N, D)}, got {d.dtype} {tuple(d.shape)}")
        if dencs[nb - 1] is not None:
            dx = dx + dencs[nb - 1]

    def injected(i):                     # block i's incoming gradient gets an exposed-output term between the calls
        return dencs is not None and 0 <= i < nb - 1 and dencs[i] is not None
    mp = pad_rows(M)
    sz, offs, tot = _bwd_sizes(B, N, D, {(run.weights[i].attn_width, run.weights[i].hidden) for i in range(nb)})
    # Workspace: the transient buffers shared by all blocks + two fp32 dx buffers that alternate + per-block SLOTS for what a deferred
    # weight-gradient job reads (bf16 g2 = the branch gradient entering the block, dh_pre, g1, dqkv): they must outlive the block's call until
    # its group is launched.  Groups of one block need two slots (block i reads g of slot i, writes the next block's into the other one).
    dxb, gb = M * D * 4, (mp * D * 2 + 255) // 256 * 256
    per = gb + sz[L.BWD_DH_PRE] + sz[L.BWD_G1] + sz[L.BWD_DQKV]
    nslots = 2 if defer.policy == "block" else nb
    ws = torch.empty(tot + 2 * dxb + nslots * per, dtype=torch.uint8, device=dev)
    base = ws.data_ptr()
    dx_ptrs = [base + tot, base + tot + dxb]
    slot0 = tot + 2 * dxb

    def slot(i):                         # byte offsets of (g, dh_pre, g1, dqkv) of block i
        o = slot0 + (i % nslots) * per
        return o, o + gb, o + gb + sz[L.BWD_DH_PRE], o + gb + sz[L.BWD_DH_PRE] + sz[L.BWD_G1]
    g_top = slot(nb - 1)[0]
    call("devit_scale_cast_bf16", ptr(dx), C.c_void_p(base + g_top), ptr(run.dps[nb - 1][1]) if run.dps is not None and run.dps[nb - 1] is not None else None,
         N, M, D, stream_ptr())
    if mp > M:
        ws[g_top + M * D * 2: g_top + mp * D * 2].zero_()
    io = L.BlockBwdIO()
    for j in range(L.BWD_COUNT):
        io.ws[j] = base + offs[j]
    io.lnws_bytes = sz[L.BWD_LNWS]
    got = (L.WgradJob * 4)()
    ngot = C.c_int(0)
    io.defer_jobs, io.defer_count = C.addressof(got), C.addressof(ngot)
    cur_dx, g_bias_done = dx.data_ptr(), 0
    st = stream_ptr()
    for i in range(nb - 1, -1, -1):
        bp = cfg.blocks[i]
        dq = dqkvs[i] if dqkvs else None
        if dq is not None:
            dq = dq.contiguous()
        out_slot = (nb - 1 - i) & 1
        og, oh, o1, oq = slot(i)
        io.dx, io.g2, io.dx_in = cur_dx, base + og, dx_ptrs[out_slot]
        io.ws[L.BWD_DH_PRE], io.ws[L.BWD_G1], io.ws[L.BWD_DQKV] = base + oh, base + o1, base + oq
        prev = cfg.blocks[i - 1] if i > 0 else None
        io.g_prev = base + slot(i - 1)[0] if prev is not None else None
        pdp = run.dps[i - 1] if (prev is not None and run.dps is not None) else None
        io.prev_dp2 = _p(pdp[1]) if pdp is not None else None
        io.prev_fc2_b_grad = grad_buf(prev.fc2_b).data_ptr() if prev is not None else None
        io.g2_bias_done = g_bias_done
        masked = run.drops is not None and run.drops[i].thr > 0        # this block masks its g2 and takes fc2's bias gradient from it
        if masked:
            io.g2_bias_done = 0
        below = (run.drops is not None and prev is not None and run.drops[i - 1].thr > 0) or injected(i - 1)
        if below:                        # ... so the block above hands it none (nor when the g it writes for the block below is rewritten)
            io.prev_fc2_b_grad = None
        io.dqkv_add = _p(dq)
        wg = _wgrads_struct(bp)
        if run.drops is not None:
            call("devit_block_bwd_drop", C.byref(run.weights[i]), C.byref(run.acts[i]), C.byref(wg), C.byref(io), C.byref(run.drops[i]), B, N, D,
                 cfg.eps, st)
        else:
            call("devit_block_bwd", C.byref(run.weights[i]), C.byref(run.acts[i]), C.byref(wg), C.byref(io), B, N, D, cfg.eps, st)
        cur_dx, g_bias_done = dx_ptrs[out_slot], 1 if (prev is not None and not below) else 0
        if injected(i - 1):
            # On `st`, behind the LayerNorm backward that wrote dx_in and g_prev and in front of everything that reads them: block i - 1's call
            # is enqueued after this launch, its weight-gradient side stream forks from an event recorded on `st` at that time
            # (csrc/encoder.hip: fork), and the deferred jobs that read this g slot are launched on `st` later still.
            add = dencs[i - 1].contiguous()
            if add.data_ptr() % 16:
                add = add.clone()
            call("devit_add_scale_cast_bf16", C.c_void_p(cur_dx), ptr(add), C.c_void_p(base + slot(i - 1)[0]), C.c_void_p(io.prev_dp2), N, M, D, st)
        defer.add(bp, [L.WgradJob.from_buffer_copy(got[k]) for k in range(ngot.value)], (dq,))
        if defer.last_of_group(i):
            defer.flush(mp)
    o = tot + (0 if cur_dx == dx_ptrs[0] else dxb)
    return ws[o:o + dxb].view(F32).view(B, N, D)


# ----------------------------------------------------------------------------------------------
# The LAST block when only the class / distillation tokens of its output are read (models/de_vit.py:286-288 takes x[:, 0], x[:, 1] after the
# final norm, and engine.py:91-92 takes q/k/v of the middle block only): one call each way (devit_tail_fwd / devit_tail_bwd, include/devit_hip.h).
# Of the last block only K and V are needed on all rows; everything else runs on the B * ntok token rows, the branch half through the block's own
# host sequence -- so the token rows, and the logits, are bit-identical to the full block's; the reference computes (and then drops) the other
# 196 rows per image.
# ----------------------------------------------------------------------------------------------
class _TailRun:
    """What the lean last block's forward leaves behind for its backward: the structs and the arena they point into."""
    __slots__ = ("weights", "acts", "arena", "x", "dims")


def _tail_forward_composite(x, bp, dp, cfg, need_grad, ntok):
    """x: fp32 [B, N, D] contiguous (output of the block before the last).  Returns (x2_tok fp32 [B, ntok, D], a view of the call's arena; the
    _TailRun).  One arena from _arena(): in a side-stream forward it lives in the consumer's pool like the body blocks' (ARENA_ALLOC_STREAM) and
    must stay referenced until the consumer has joined (EncoderFn.forward hangs it on the last body block's qkv view)."""
    B, N, D = x.shape
    run = _TailRun()
    w = run.weights = _weights_struct(bp)
    if w.dtype16 and need_grad:
        raise L.DevitError('precision="f16" is forward-only (frozen teacher): run it under torch.no_grad()')
    flags = L.BLK_SAVE if need_grad else 0
    sz, offs, tot = _sizes("devit_tail_acts_sizes", L.TAIL_ACT_COUNT, B, N, ntok, D, w.attn_width, w.hidden, flags)
    run.arena, run.x, run.dims = _arena(tot, x.device), x, (B, N, D)
    base = run.arena.data_ptr()
    t = run.acts = L.TailActs()
    t.acts.x, t.acts.flags, t.ntok = x.data_ptr(), flags, ntok
    for j in range(L.ACT_COUNT):
        t.acts.buf[j] = base + offs[j] if sz[j] else None
    t.ln1_tok, t.q, t.x_tok = (base + offs[j] for j in (L.TAIL_LN1_TOK, L.TAIL_Q, L.TAIL_X_TOK))
    t.acts.dp1, t.acts.dp2 = (_p(dp[0]), _p(dp[1])) if dp is not None else (None, None)
    call("devit_tail_fwd", C.byref(w), C.byref(t), B, N, D, cfg.eps, stream_ptr())
    if getattr(bp, "module", None) is not None:
        # the shrink contract's debug views (models/de_vit.py:41,77) of THIS block are not produced on the lean path: drop the ones an
        # earlier full forward left, so a ranking pass run inside lean_tail fails loudly instead of reading stale activations (and the
        # arena they kept alive is released)
        bp.module.mlp.neuron_output = None
        bp.module.attn.head_output = None
    o = offs[L.ACT_X2]
    return run.arena[o:o + B * ntok * D * 4].view(F32).view(B, ntok, D), run


def _tail_backward_composite(run, bp, cfg, dx, defer=None):
    """dx: fp32 [B, ntok, D] gradient of _tail_forward_composite's output.  Returns the fp32 [B, N, D] gradient of its input, a view of the call's
    workspace.  defer: a DeferredWgrads whose single group is launched behind block 0 -- the one product of this block that reduces over ALL rows
    (dK | dV against ln1) then rides that launch as a job, and the caller reports this block with that group."""
    B, N, D = run.dims
    w, ntok = run.weights, run.acts.ntok
    T, M = B * ntok, B * N
    sz, offs, tot = _sizes("devit_tail_bwd_sizes", L.TAIL_BWD_COUNT, B, N, ntok, D, w.attn_width, w.hidden)
    gb = (pad_rows(T) * D * 2 + 255) // 256 * 256
    ws = torch.empty(tot + gb + M * D * 4, dtype=torch.uint8, device=dx.device)        # transients, g2 = bf16(dp2 * dx), dx_in
    base = ws.data_ptr()
    dx = dx.contiguous()
    call("devit_scale_cast_bf16", ptr(dx), C.c_void_p(base + tot), C.c_void_p(run.acts.acts.dp2), ntok, T, D, stream_ptr())
    io = L.TailBwdIO()
    io.dx, io.g2, io.dx_in, io.lnws_bytes = dx.data_ptr(), base + tot, base + tot + gb, sz[L.BWD_LNWS]
    for j in range(L.TAIL_BWD_COUNT):
        io.ws[j] = base + offs[j]
    got, ngot = L.WgradJob(), C.c_int(0)
    if defer is not None:
        io.defer_jobs, io.defer_count = C.addressof(got), C.addressof(ngot)
    wg = _wgrads_struct(bp)
    call("devit_tail_bwd", C.byref(w), C.byref(run.acts), C.byref(wg), C.byref(io), B, N, D, cfg.eps, stream_ptr())
    if defer is not None:      # (the job reads DKV of the workspace and LN1 of the arena: both stay until the group is launched)
        defer.add(bp, [L.WgradJob.from_buffer_copy(got)] if ngot.value else [], (ws, run.arena, grad_buf(bp.qkv_w), grad_buf(bp.qkv_b)))
    o = tot + gb
    return ws[o:o + M * D * 4].view(F32).view(B, N, D)


class EncoderFn(torch.autograd.Function):
    """x -> blocks[0..n) -> (x_out, [qkv_i bf16 packed ...], [att_i ...], [enc_i ...])."""

    @staticmethod
    def forward(ctx, x, cfg, *params):
        L.require_device(x)
        x = x.contiguous()
        need_grad = cfg.grad_enabled and (x.requires_grad or any(p is not None and p.requires_grad for p in params))
        if need_grad and any(getattr(bp, "compacted", False) and getattr(bp, "masters", None) is None for bp in cfg.blocks):
            raise L.DevitError("this model was compacted for inference (shrink.compact(model)): run it under torch.no_grad(), "
                               "or compact it with shrink.compact(model, trainable=True) to train through the compacted blocks")
        nb = len(cfg.blocks)
        # lean tail (EncoderCfg.lean_tokens): the last block runs on the token rows only
        # (with an enc_layers selector the tail stays lean unless the last block's output is one of those handed out)
        enc_sel = cfg.enc_layers if cfg.want_enc else None
        enc_last = cfg.want_enc and (enc_sel is None or nb - 1 in enc_sel)
        lean = cfg.lean_tokens if (cfg.lean_tokens and nb >= 2 and not cfg.want_att and not enc_last and cfg.drop is None) else 0
        nbody = nb - 1 if lean else nb
        dp_last = cfg.dp_scales[nb - 1] if cfg.dp_scales is not None else None
        ctx.tail = None
        run = _encoder_forward_composite(x, cfg, need_grad, nbody)
        qkvs = [v["qkv"] for v in run.views] if cfg.want_qkv else []
        atts = [v["att"] for v in run.views] if cfg.want_att else []
        if cfg.want_enc and enc_sel is not None:      # the selected blocks' outputs, None for the others (the lean last block is never selected)
            encs = [None if i not in enc_sel else run.views[i]["x2"].clone() if i == nb - 1 else run.views[i]["x2"] for i in range(nb)]
        else:
            encs = [run.views[i]["x2"].clone() if i == nb - 1 else run.views[i]["x2"] for i in range(nb)] if cfg.want_enc else []
        ctx.cfg, ctx.need_grad = cfg, need_grad
        ctx.run = run if need_grad else None
        ctx.counts = (len(qkvs), len(atts), len(encs))
        # outputs nobody differentiates (11 of the 12 qkv tensors in the DEKD step) arrive as None in backward, not as
        # zero tensors: a materialised one is a 117 MB fill plus a 117 MB read in the attention backward, per block
        ctx.set_materialize_grads(False)
        xo = run.views[-1]["x2"]
        if lean:
            xo, tail = _tail_forward_composite(xo, cfg.blocks[-1], dp_last, cfg, need_grad, lean)
            ctx.tail = tail if need_grad else None
            if ARENA_ALLOC_STREAM is not None and qkvs:      # a side-stream forward's arenas stay referenced by the returned dict until the consumer
                qkvs[-1]._devit_tail_arena = tail.arena       # has joined: this block hands out no view of its own to hold its arena
        return (xo,) + tuple(qkvs) + tuple(atts) + tuple(encs)

    @staticmethod
    def backward(ctx, dx, *dothers):
        cfg = ctx.cfg
        if not ctx.need_grad:
            raise L.DevitError("EncoderFn.backward called but the forward ran without grad bookkeeping")
        nq, na, ne = ctx.counts
        dqkvs, datts, dencs = dothers[:nq], dothers[nq:nq + na], dothers[nq + na:]
        if any(d is not None for d in datts):
            raise L.DevitError("gradients into the exposed 'attention' outputs are not taken on the 16-bit path: "
                               'run the model with precision="f32" (ops_f32.EncoderF32Fn implements them)')
        nb = len(cfg.blocks)
        nparams = 12 * nb
        if ctx.tail is not None:          # lean tail: dx is the [B, ntok, D] gradient of the token rows
            tail, ctx.tail = ctx.tail, None
            last = cfg.blocks[-1]
            if dx is None:
                dx = torch.zeros((tail.dims[0], tail.acts.ntok, tail.dims[2]), dtype=F32, device=tail.x.device)
            nb -= 1
            defer = DeferredWgrads(cfg, nb)
            if defer.policy == "all":          # (no exchange to overlap: the last block is reported with the one group)
                dx = _tail_backward_composite(tail, last, cfg, dx, defer)
            else:
                dx = _tail_backward_composite(tail, last, cfg, dx)
                last.finish_grads()
                if cfg.grad_ready is not None:
                    cfg.grad_ready(last.all_params())
        else:
            defer = DeferredWgrads(cfg, nb)
        run, ctx.run = ctx.run, None
        B, N, D = run.dims
        if dx is None:
            dx = torch.zeros((B, N, D), dtype=F32, device=run.x.device)
        # (a lean forward hands out no output of its last block: dencs[nb] is None there, and the body's top block is nb - 1)
        dx_in = _encoder_backward_composite(run, cfg, dx.contiguous(), dqkvs if nq else None, defer, list(dencs[:nb]) if ne else None)
        return (dx_in, None) + (None,) * nparams


# ----------------------------------------------------------------------------------------------
# patch embedding + token assembly (models/de_vit.py:258-264)
# ----------------------------------------------------------------------------------------------
IMG_SIZES = tuple(range(32, 225, 16))      # square image sides the patch-cutting kernels are built for (csrc/devit_common.h): grids 2 x 2 .. 14 x 14


def check_img_size(img_size, patch_size=16, in_chans=3, exc=NotImplementedError):
    """The side S of a supported image geometry -- square, 3 channels, 16 x 16 patches, S in IMG_SIZES -- or `exc` with the reason.
    224 is the ceiling: the next size, 240 pixels, is 225 patches + 2 tokens = 227 rows, over the 208 the attention kernels hold."""
    hw = tuple(img_size) if isinstance(img_size, (tuple, list)) else (img_size, img_size)
    ps = tuple(patch_size) if isinstance(patch_size, (tuple, list)) else (patch_size, patch_size)
    if len(hw) != 2 or hw[0] != hw[1]:
        raise exc(f"image size {img_size}: the patch-embed kernels are built for square images (one of {list(IMG_SIZES)})")
    if ps != (16, 16) or in_chans != 3:
        raise exc(f"patch size {patch_size}, {in_chans} channels: the patch-embed kernels are built for 16 x 16 patches of 3-channel images")
    S = hw[0]
    if S not in IMG_SIZES:
        why = ("240 pixels are 15 x 15 patches + 2 tokens = 227 rows, over the 208 the attention kernels hold" if isinstance(S, int) and S > 224
               else "a multiple of 16, at least two patches a side")
        raise exc(f"image size {S}: the patch-embed kernels are built for {list(IMG_SIZES)} ({why})")
    return S


def image_side(img, what):
    """S of an fp32 image batch [B,3,S,S] (or of PatchRows), DevitError for a shape the patch-cutting kernels do not take."""
    shape = tuple(img.shape)
    if len(shape) != 4 or shape[0] < 1:
        raise L.DevitError(f"{what}: expected images [B,3,S,S], got {shape}")
    return check_img_size(shape[2:], 16, shape[1], exc=lambda m: L.DevitError(f"{what}: got {shape}: {m}"))


def expect_side(x, S, what):
    """A model built for S x S images refuses a batch (images or PatchRows) of another size: the kernels would run off the buffers."""
    got = image_side(x, what)
    if got != S:
        raise L.DevitError(f"{what}: the model is built for {S} x {S} images (img_size={S}), the batch is {got} x {got} {tuple(x.shape)}")
    return got


class PatchRows:
    """A batch of images already cut into bf16 patch rows [pad_rows(B*T), 768] (k = c*256 + kh*16 + kw; T = grid^2 patches of
    an img_size x img_size image, 196 at 224): what every
    model's patch-embedding GEMM reads.  Models accept it in place of the fp32 image tensor, so one im2row pass -- plain
    (`patch_rows`) or fused with Mixup / CutMix (`mix_patch_rows`) -- serves the student, the teacher and all MultiViT
    backbones of a step.  Quacks like the image batch where host code only asks for its size and place."""

    def __init__(self, rows, B, rows_f16=None, img_size=224):
        self.rows, self.rows_f16, self.B = rows, rows_f16, B          # bf16 rows and / or the same values in IEEE f16
        self.img_size = check_img_size(img_size)
        self.grid = self.img_size // 16
        self.num_patches = self.grid * self.grid
        self.shape = (B, 3, self.img_size, self.img_size)

    _any = property(lambda self: self.rows if self.rows is not None else self.rows_f16)
    is_cuda = property(lambda self: self._any.is_cuda)
    device = property(lambda self: self._any.device)
    dtype = torch.float32

    def of(self, dtype):
        t = self.rows_f16 if dtype == F16 else self.rows
        if t is None:
            raise L.DevitError(f"PatchRows holds no {dtype} rows: build them with patch_rows(img, dtypes=...) / "
                               "mix_patch_rows(..., dtypes=...) for every precision the models of the step run in")
        return t

    def record_stream(self, s):
        for t in (self.rows, self.rows_f16):
            if t is not None:
                t.record_stream(s)


PATCH_ROW_DTYPES = (torch.bfloat16,)      # what patch_rows / mix_patch_rows produce by default


def patch_rows(img, dtypes=None):
    """fp32 [B,3,S,S] (S in IMG_SIZES) -> PatchRows (devit_im2row_bf16); dtypes: which 16-bit copies to make (bf16 and / or f16)."""
    if isinstance(img, PatchRows):
        return img
    L.require_device(img)
    S = image_side(img, "patch_rows")
    img = img.contiguous().float()
    B, T = img.shape[0], (S // 16) ** 2
    out = {}
    for dt in (dtypes or PATCH_ROW_DTYPES):
        out[dt] = rows_alloc(B * T, 768, dt, img.device)
        call("devit_im2row_bf16", ptr(img), ptr(out[dt]), B, 3, S, S, 16, int(dt == F16), stream_ptr())
    return PatchRows(out.get(torch.bfloat16), B, out.get(F16), S)


def mix_patch_rows(img, mode, lam=1.0, box=(0, 0, 0, 0), dtypes=None):
    """Mixup (mode 1) / CutMix (mode 2, box = (y0, y1, x0, x1)) of a batch with its flip, straight to patch rows
    (devit_mix_im2row_bf16_sized; timm Mixup mode='batch', engine.py:65-66).  The box lies inside the S x S image."""
    L.require_device(img)
    S = image_side(img, "mix_patch_rows")
    img = img.contiguous().float()
    B, T = img.shape[0], (S // 16) ** 2
    dtypes = dtypes or PATCH_ROW_DTYPES
    rows = rows_alloc(B * T, 768, torch.bfloat16, img.device) if torch.bfloat16 in dtypes else None
    rows_h = rows_alloc(B * T, 768, F16, img.device) if F16 in dtypes else None
    call("devit_mix_im2row_bf16_sized", ptr(img), ptr(rows), ptr(rows_h), B, int(mode), float(lam), int(box[0]), int(box[1]),
         int(box[2]), int(box[3]), S, S, stream_ptr())
    return PatchRows(rows, B, rows_h, S)


def mix_targets(labels, num_classes, lam, smoothing):
    """[B, C] soft targets of the mixed batch (timm mixup_target)."""
    L.require_device(labels)
    labels = labels.contiguous().long()
    out = torch.empty((labels.shape[0], num_classes), dtype=F32, device=labels.device)
    call("devit_mix_targets", ptr(labels), ptr(out), labels.shape[0], num_classes, float(lam), float(smoothing), stream_ptr())
    return out


# ---- per-sample Mixup / CutMix (timm Mixup mode='elem' / 'pair'): one devit_mix_sample per image ----
# host mirror of devit_mix_sample (32 bytes, _lib.MixSample): what Mixup.draw_table fills and mix_table uploads
MIX_SAMPLE_DTYPE = np.dtype([("mode", "<i4"), ("lam", "<f4"), ("y0", "<i4"), ("y1", "<i4"), ("x0", "<i4"), ("x1", "<i4"),
                             ("reserved", "<i4", (2,))])
MIX_RING_SLOTS = 256
_mix_ring = {}        # device -> [pinned uint8 [MIX_RING_SLOTS, bytes per slot], uploads so far]


class MixTable:
    """A validated table of B devit_mix_sample entries: `host` (numpy, MIX_SAMPLE_DTYPE) and its copy on the device, `dev` (uint8)."""

    def __init__(self, host, dev, img_size=224):
        self.host, self.dev, self.B, self.img_size = host, dev, host.shape[0], img_size      # img_size: what the boxes were checked against


def mix_entries(entries, img_size=224):
    """A numpy structured array with the fields of MIX_SAMPLE_DTYPE, or a list of (mode, lam, y0, y1, x0, x1) -> a validated
    MIX_SAMPLE_DTYPE array.  ValueError for a mode outside {0, 1, 2}, lam outside [0, 1] or NaN, a box outside
    0 <= lo <= hi <= img_size (224 unless given), or mode 0 with lam != 1 (the images would stay as they are and the targets would not).  The kernels
    are memory-safe for any table bytes and the C entry cannot read device memory, so this is where the values are checked."""
    if isinstance(entries, np.ndarray) and entries.dtype.names:
        cols = [np.asarray(entries[n]).reshape(-1) for n in ("mode", "lam", "y0", "y1", "x0", "x1")]
    else:
        rows = [tuple(e) for e in entries]
        if any(len(r) != 6 for r in rows):
            raise ValueError("mix_table: an entry is (mode, lam, y0, y1, x0, x1)")
        cols = [np.asarray(c) for c in zip(*rows)] if rows else [np.zeros(0)] * 6
    mode, lam, y0, y1, x0, x1 = cols
    if mode.shape[0] < 1:
        raise ValueError("mix_table: empty table")
    lam = lam.astype(np.float64)
    if not np.isin(mode, (0, 1, 2)).all():
        raise ValueError(f"mix_table: mode must be 0 (none), 1 (mixup) or 2 (cutmix), got {sorted(set(mode.tolist()) - {0, 1, 2})}")
    if not ((lam >= 0) & (lam <= 1)).all():             # (a NaN compares false)
        raise ValueError(f"mix_table: lam must lie in [0, 1], got {lam[~((lam >= 0) & (lam <= 1))].tolist()}")
    for lo, hi, ax in ((y0, y1, "y"), (x0, x1, "x")):
        bad = ~((0 <= lo) & (lo <= hi) & (hi <= img_size))
        if bad.any():
            i = int(np.flatnonzero(bad)[0])
            raise ValueError(f"mix_table: entry {i}: box [{lo[i]}, {hi[i]}) on {ax} is not inside 0 <= lo <= hi <= {img_size}")
    if ((mode == 0) & (lam != 1)).any():
        raise ValueError("mix_table: a mode 0 entry carries lam != 1: its image stays as it is, so its target must too")
    host = np.zeros(mode.shape[0], dtype=MIX_SAMPLE_DTYPE)
    for n, c in zip(("mode", "lam", "y0", "y1", "x0", "x1"), (mode, lam, y0, y1, x0, x1)):
        host[n] = c
    return host


def mix_table(entries, device="cuda", img_size=224):
    """entries (see mix_entries) -> MixTable on `device` for img_size x img_size images.  ValueError, before anything touches the device, for a mode outside
    {0, 1, 2}, lam outside [0, 1] or NaN, a box outside 0 <= lo <= hi <= img_size, and mode 0 with lam != 1.  The upload is an async copy
    out of a pinned ring and never waits for the stream: the host runs steps ahead of the GPU, so every table in flight has a slot of
    its own (as optim.FlatAdamW's scalars).  No event guards a slot: the ring holds MIX_RING_SLOTS = 256 uploads, and a caller more
    than 255 uploads ahead of the stream (one upload per training step) would overwrite a table still in flight."""
    img_size = check_img_size(img_size, exc=ValueError)
    host = mix_entries(entries, img_size)
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:      # 'cuda' and 'cuda:N' of the current device share one ring
        device = torch.device("cuda", torch.cuda.current_device())
    nbytes = host.nbytes
    ring = _mix_ring.get(device)
    if ring is None or ring[0].shape[1] < nbytes:
        # (a ring that was outgrown is dropped, not reused: the pinned allocator keeps it until the copies out of it are done)
        ring = _mix_ring[device] = [torch.zeros((MIX_RING_SLOTS, max(nbytes, 8192)), dtype=torch.uint8).pin_memory(), 0]
    slot = ring[0][ring[1] % MIX_RING_SLOTS, :nbytes]
    ring[1] += 1
    slot.copy_(torch.from_numpy(host.view(np.uint8)))
    dev = torch.empty(nbytes, dtype=torch.uint8, device=device)
    dev.copy_(slot, non_blocking=True)
    return MixTable(host, dev, img_size)


def _table_for(table, B, img_size=None):
    if not isinstance(table, MixTable):
        raise TypeError("expected the MixTable that ops.mix_table returns")
    if table.B != B:
        raise ValueError(f"the table has {table.B} entries, the batch {B} samples")
    if img_size is not None and table.img_size != img_size:       # its boxes were checked against another image
        raise ValueError(f"the table was built for {table.img_size} x {table.img_size} images (ops.mix_table(img_size=...)), the batch is "
                         f"{img_size} x {img_size}")
    return table


def mix_patch_rows_table(img, table, dtypes=None, f32_images=False):
    """Per-sample Mixup / CutMix of a batch with its flip (sample b with B-1-b, entry b of `table`), straight to patch rows
    (devit_mix_im2row_table_sized) -> PatchRows; f32_images: the mixed batch as a NEW fp32 [B,3,S,S] tensor instead (what an
    "f32" model reads).  `img` itself is only read; the table is one built for this image size (ops.mix_table(img_size=S))."""
    L.require_device(img)
    S = image_side(img, "mix_patch_rows_table")
    img = img.contiguous().float()
    B, T = img.shape[0], (S // 16) ** 2
    table = _table_for(table, B, S)
    if f32_images:
        out = torch.empty_like(img)
        call("devit_mix_im2row_table_sized", ptr(img), None, None, ptr(out), ptr(table.dev), B, S, S, stream_ptr())
        return out
    dtypes = dtypes or PATCH_ROW_DTYPES
    rows = rows_alloc(B * T, 768, torch.bfloat16, img.device) if torch.bfloat16 in dtypes else None
    rows_h = rows_alloc(B * T, 768, F16, img.device) if F16 in dtypes else None
    call("devit_mix_im2row_table_sized", ptr(img), ptr(rows), ptr(rows_h), None, ptr(table.dev), B, S, S, stream_ptr())
    return PatchRows(rows, B, rows_h, S)


def mix_targets_table(labels, num_classes, table, smoothing):
    """[B, C] soft targets of the batch mixed per sample: row b = lam_b * smooth(y[b]) + (1 - lam_b) * smooth(y[B-1-b])
    (timm mixup_target with a [B, 1] float32 lam)."""
    L.require_device(labels)
    labels = labels.contiguous().long()
    table = _table_for(table, labels.shape[0])
    out = torch.empty((labels.shape[0], num_classes), dtype=F32, device=labels.device)
    call("devit_mix_targets_table", ptr(labels), ptr(out), ptr(table.dev), labels.shape[0], num_classes, float(smoothing), stream_ptr())
    return out


class PatchEmbedFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, img, proj_w, proj_b, cls_token, dist_token, pos_embed, w16, grad_ready):
        pre = img if isinstance(img, PatchRows) else patch_rows(img, (w16.dtype,))
        rows, B = pre.of(w16.dtype), pre.B
        dev = rows.device
        D = proj_w.shape[0]
        ntok = 2 if dist_token is not None else 1
        T = pos_embed.shape[1]                  # tokens of the MODEL: its patches + ntok
        P = T - ntok
        if pre.num_patches != P:                # (VisionTransformer.embed names both sizes before it gets here)
            raise L.DevitError(f"PatchEmbedFn: pos_embed holds {P} patch positions, the batch {tuple(pre.shape)} has {pre.num_patches} patches")
        M = B * P
        x = torch.empty((B, T, D), dtype=F32, device=dev)
        gemm(rows, 768, 0, w16, 768, 0, pad_rows(M), D, 768, kind=L.EPI_PATCH_F32, out=x, ldc=D, bias=proj_b,
             pos=pos_embed, patch_tokens=P, extra_tokens=ntok, m_valid=M, dtype16=int(w16.dtype == F16))
        call("devit_embed_tokens", ptr(cls_token), ptr(dist_token), ptr(pos_embed), ptr(x), B, T, D, stream_ptr())
        ctx.rows, ctx.dims = rows, (B, T, D, ntok)
        ctx.params = (proj_w, proj_b, cls_token, dist_token, pos_embed)
        ctx.grad_ready = grad_ready
        return x

    @staticmethod
    def backward(ctx, dx):
        B, T, D, ntok = ctx.dims
        proj_w, proj_b, cls_token, dist_token, pos_embed = ctx.params
        dx = dx.contiguous()
        dev = dx.device
        # bf16 copy of dx with pad rows (the wgrad reduces over padded patch rows; skipped rows map past the end: the last reduction row
        # pad_rows(B * P) - 1 lives at physical row r + ntok * (r / P + 1), which with few patches per image -- P = 4 at 32 pixels -- lies
        # well behind the 128 spare rows that cover 224-pixel batches)
        P = T - ntok
        last = pad_rows(B * P) - 1
        dxb = rows_alloc(B * T, D, BF16, dev, extra=max(128, last + ntok * (last // P + 1) + 1 - pad_rows(B * T)))
        dpos = torch.empty((T, D), dtype=F32, device=dev)
        dcls = torch.empty(D, dtype=F32, device=dev)
        ddist = torch.empty(D, dtype=F32, device=dev) if ntok == 2 else None
        dbias = torch.empty(D, dtype=F32, device=dev)
        call("devit_embed_bwd", ptr(dx), B, T, D, ntok, ptr(dpos), ptr(dcls), ptr(ddist), ptr(dbias), ptr(dxb), 0,
             stream_ptr())
        grad_buf(pos_embed).view(T, D).add_(dpos)
        grad_buf(cls_token).view(D).add_(dcls)
        if ntok == 2:
            grad_buf(dist_token).view(D).add_(ddist)
        grad_buf(proj_b).add_(dbias)
        # dW[D, 768] += dx_patch^T @ rows ; reduction row r=(b,t) lives at physical row r + ntok*(r/P + 1), P = T - ntok patches
        M = B * P
        mp = pad_rows(M)
        gemm(dxb, D, 1, ctx.rows, 768, 1, D, 768, mp, kind=L.EPI_ATOMIC_F32, out=grad_buf(proj_w), ldc=768,
             split_k=split_k_for(D, 768, mp // 64), a_group=P, a_skip=ntok)
        if ctx.grad_ready is not None:
            ctx.grad_ready([p for p in ctx.params if p is not None])
        return (None,) * 8


# ----------------------------------------------------------------------------------------------
# final norm on the cls/dist rows + classifier heads (models/de_vit.py:286-288,316-318)
# ----------------------------------------------------------------------------------------------
class PosDropFn(torch.autograd.Function):
    """pos_drop (models/de_vit.py:173,264) on the fp32 token stream [B, T, D]: site 0, block 0 of the forward's seed; the backward regenerates the mask."""

    @staticmethod
    def forward(ctx, x, seed, p):
        from . import dropout
        L.require_device(x)
        B, T, D = x.shape
        y = x.contiguous().clone()
        dropout.apply_(y.view(B * T, D), B * T, seed, L.DROP_POS, 0, p)
        ctx.key = (seed, p)
        return y

    @staticmethod
    def backward(ctx, dy):
        from . import dropout
        B, T, D = dy.shape
        dx = dy.contiguous().clone()
        dropout.apply_(dx.view(B * T, D), B * T, ctx.key[0], L.DROP_POS, 0, ctx.key[1])
        return dx, None, None


class HeadsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, norm_w, norm_b, head_w, head_b, headd_w, headd_b, ntok, eps, grad_ready):
        L.require_device(x)
        x = x.contiguous()
        B, T, D = x.shape
        rows = B * ntok
        dev = x.device
        tok = torch.empty((B, ntok, D), dtype=F32, device=dev)
        mean = torch.empty(rows, dtype=F32, device=dev)
        rstd = torch.empty(rows, dtype=F32, device=dev)
        layernorm_fwd(x.view(B * T, D), rows, D, norm_w, norm_b, eps, y_f32=tok, mean=mean, rstd=rstd, in_group=ntok,
                      in_stride=T)
        outs = [tok]
        if head_w is not None:
            Cn = head_w.shape[0]
            lo = torch.empty((B, Cn), dtype=F32, device=dev)
            sgemm_small(tok, ntok * D, 1, head_w, D, 1, head_b, lo, Cn, B, Cn, D)
            outs.append(lo)
            if ntok == 2 and headd_w is not None:
                lk = torch.empty((B, Cn), dtype=F32, device=dev)
                sgemm_small(tok[:, 1], ntok * D, 1, headd_w, D, 1, headd_b, lk, Cn, B, Cn, D)
                outs.append(lk)
        ctx.save = (x, tok, mean, rstd)
        ctx.params = (norm_w, norm_b, head_w, head_b, headd_w, headd_b)
        ctx.meta = (B, T, D, ntok, eps, grad_ready)
        ctx.set_materialize_grads(False)
        return tuple(outs)

    @staticmethod
    def backward(ctx, dtok, dlo=None, dlk=None):
        # (released here, like EncoderFn's: `tok` is an output of this node, so ctx.save is a reference cycle that only the garbage collector would
        # free -- and x, a view of the lean last block's arena, would keep that arena allocated until then)
        (x, tok, mean, rstd), ctx.save = ctx.save, None
        norm_w, norm_b, head_w, head_b, headd_w, headd_b = ctx.params
        B, T, D, ntok, eps, grad_ready = ctx.meta
        dev = x.device
        dt = torch.zeros((B, ntok, D), dtype=F32, device=dev) if dtok is None else dtok.contiguous().clone()
        for j, (dl, w, b) in enumerate(((dlo, head_w, head_b), (dlk, headd_w, headd_b))):
            if dl is None or w is None:
                continue
            dl = dl.contiguous()
            Cn = w.shape[0]
            # dtok_j[B, D] += dl[B, C] @ w[C, D]
            sgemm_small(dl, Cn, 1, w, 1, D, None, dt[:, j], ntok * D, B, D, Cn, accumulate=True)
            # dw[C, D] += dl^T @ tok_j ; db += colsum(dl)
            sgemm_small(dl, 1, Cn, tok[:, j], 1, ntok * D, None, grad_buf(w), D, Cn, D, B, accumulate=True)
            ones = _ones1(dev)
            sgemm_small(dl, 1, Cn, ones, 0, 0, None, grad_buf(b), 1, Cn, 1, B, accumulate=True)
        dx = torch.zeros((B, T, D), dtype=F32, device=dev)
        layernorm_bwd(dt, True, x.view(B * T, D), B * ntok, D, mean, rstd, norm_w, None, dx.view(B * T, D), None, None,
                      0, grad_buf(norm_w), grad_buf(norm_b), in_group=ntok, in_stride=T)
        if grad_ready is not None:
            grad_ready([p for p in ctx.params if p is not None])
        return (dx,) + (None,) * 9


# ----------------------------------------------------------------------------------------------
# stand-alone Mlp / Attention nodes (module-level API of models/de_vit.py:21-87; the model path
# runs whole blocks through EncoderFn)
# ----------------------------------------------------------------------------------------------
def _to_rows_bf16(x):
    B, N, D = x.shape
    M = B * N
    buf = rows_alloc(M, D, BF16, x.device)
    call("devit_scale_cast_bf16", ptr(x.contiguous().float()), ptr(buf), None, 0, M, D, stream_ptr())
    return buf


class MlpFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, module, w1, b1, w2, b2, w1_16, w2_16, gate, grad_enabled):
        L.require_device(x)
        B, N, D = x.shape
        M, dev, Hd, Do = B * N, x.device, w1.shape[0], w2.shape[0]
        xb = _to_rows_bf16(x)
        need = grad_enabled and (x.requires_grad or w1.requires_grad)
        h = rows_alloc(M, Hd, BF16, dev)
        h_pre = rows_alloc(M, Hd, BF16, dev) if need else None
        linear_fwd(xb, w1_16, b1, M, out=h, kind=L.EPI_GELU_BF16, colscale=gate, aux=h_pre, exact_gelu=0)
        y = torch.empty((B, N, Do), dtype=F32, device=dev)
        linear_fwd(h, w2_16, b2, M, out=y.view(M, Do), kind=L.EPI_STORE_F32)
        module.neuron_output = h[:M].view(B, N, Hd)
        ctx.s = (xb, h, h_pre, gate, w1, b1, w2, b2, w1_16, w2_16, (B, N, D))
        return y

    @staticmethod
    def backward(ctx, dy):
        xb, h, h_pre, gate, w1, b1, w2, b2, w1_16, w2_16, (B, N, D) = ctx.s
        M, dev, Hd = B * N, dy.device, w1.shape[0]
        g = _to_rows_bf16(dy)
        dh = rows_alloc(M, Hd, BF16, dev)
        linear_dgrad(g, w2_16, M, out=dh, kind=L.EPI_DGELU_BF16, colscale=gate, aux_in=h_pre)
        linear_wgrad(g, h, grad_buf(w2), grad_buf(b2), M)
        dx = torch.empty((B, N, D), dtype=F32, device=dev)
        linear_dgrad(dh, w1_16, M, out=dx.view(M, D), kind=L.EPI_STORE_F32)
        linear_wgrad(dh, xb, grad_buf(w1), grad_buf(b1), M)
        return (dx,) + (None,) * 9


class AttentionFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, module, wq, bq, wp, bp_, wq16, wp16, gate, grad_enabled):
        L.require_device(x)
        B, N, D = x.shape
        M, dev, H = B * N, x.device, module.num_heads
        xb = _to_rows_bf16(x)
        need = grad_enabled and (x.requires_grad or wq.requires_grad)
        qkv = rows_alloc(M, 3 * D, BF16, dev)
        linear_fwd(xb, wq16, bq, M, out=qkv)
        o = rows_alloc(M, D, BF16, dev)
        lse = torch.empty((B, H, N), dtype=F32, device=dev) if need else None
        call("devit_attn_fwd", ptr(qkv), ptr(o), ptr(lse), ptr(gate), B, N, H, D // H, (D // H) ** -0.5, 0, stream_ptr())
        y = torch.empty((B, N, D), dtype=F32, device=dev)
        linear_fwd(o, wp16, bp_, M, out=y.view(M, D), kind=L.EPI_STORE_F32)
        module.head_output = o[:M].view(B, N, H, D // H)
        ctx.s = (xb, qkv, o, lse, gate, wq, bq, wp, bp_, wq16, wp16, (B, N, D, H))
        return y, qkv

    @staticmethod
    def backward(ctx, dy, dqkv_in):
        xb, qkv, o, lse, gate, wq, bq, wp, bp_, wq16, wp16, (B, N, D, H) = ctx.s
        M, dev = B * N, dy.device
        g = _to_rows_bf16(dy)
        do = rows_alloc(M, D, BF16, dev)
        linear_dgrad(g, wp16, M, out=do)
        linear_wgrad(g, o, grad_buf(wp), grad_buf(bp_), M)
        dqkv = rows_alloc(M, 3 * D, BF16, dev)
        call("devit_attn_bwd", ptr(qkv), ptr(o), ptr(do), ptr(lse), ptr(gate),
             ptr(dqkv_in.contiguous()) if dqkv_in is not None else None, ptr(dqkv), B, N, H, D // H, (D // H) ** -0.5,
             stream_ptr())
        dx = torch.empty((B, N, D), dtype=F32, device=dev)
        linear_dgrad(dqkv, wq16, M, out=dx.view(M, D), kind=L.EPI_STORE_F32)
        linear_wgrad(dqkv, xb, grad_buf(wq), grad_buf(bq), M)
        return (dx,) + (None,) * 9


# ----------------------------------------------------------------------------------------------
# losses
# ----------------------------------------------------------------------------------------------
class ClsDistillLossFn(torch.autograd.Function):
    """utils/losses.py:156-177 with a SoftTargetCrossEntropy base criterion; loss + gradient in one launch."""

    @staticmethod
    def forward(ctx, logits, logits_kd, teacher_logits, soft_targets, kind, alpha, tau):
        L.require_device(logits)
        logits, logits_kd = logits.contiguous().float(), logits_kd.contiguous().float()
        soft_targets = soft_targets.contiguous().float()
        tl = teacher_logits.contiguous().float() if teacher_logits is not None else None
        B, Cn = logits.shape
        loss3 = torch.empty(3, dtype=F32, device=logits.device)
        dlo, dlk = torch.empty_like(logits), torch.empty_like(logits_kd)
        call("devit_cls_distill_loss", ptr(logits), ptr(logits_kd), ptr(tl), ptr(soft_targets), B, Cn,
             {"none": 0, "soft": 1, "hard": 2}[kind], alpha, tau, ptr(loss3), ptr(dlo), ptr(dlk), stream_ptr())
        ctx.save_for_backward(dlo, dlk)
        return loss3[0]

    @staticmethod
    def backward(ctx, g):
        dlo, dlk = ctx.saved_tensors
        return dlo * g, dlk * g, None, None, None, None, None


def relation_fused_selected(s_qkv, t_qkv, B, N):
    """Does RelationLossFn run csrc/relation.hip's two launches for these packed buffers?  N <= 208, both widths multiples of 64 up to 1024, a bf16
    student and a bf16 or f16 teacher buffer holding the B N rows, and DEVIT_RELFUSE (read per call) not 0."""
    if os.environ.get("DEVIT_RELFUSE", "") == "0":
        return False
    Ds, Dt = s_qkv.shape[1] // 3, t_qkv.shape[1] // 3
    return (s_qkv.dtype == BF16 and t_qkv.dtype in (BF16, F16) and 0 < N <= 208 and B > 0
            and all(0 < D <= 1024 and D % 64 == 0 for D in (Ds, Dt))
            and all(b.dim() == 2 and b.shape[1] == 3 * D and b.stride(1) == 1 and b.stride(0) % 8 == 0 and b.shape[0] >= B * N
                    and b.data_ptr() % 16 == 0 for b, D in ((s_qkv, Ds), (t_qkv, Dt))))


class RelationLossFn(torch.autograd.Function):
    """q/k/v feature-relation losses (utils/losses.py:307-328) on PACKED qkv buffers.

    t_qkv: bf16 [>= B*N + 58 rows, 3*Dt], s_qkv likewise with Ds; component j lives in columns [j*D, (j+1)*D).
    Returns fp32 [3] = (q, k, v) losses.  Gradient flows to the student buffer only.

    Where relation_fused_selected() says so the two launches of csrc/relation.hip run (Grams on chip; the context keeps the bf16 S_unit of the
    three components and nothing else); otherwise the batched GEMMs around devit_relation_stats / devit_relation_grad."""

    @staticmethod
    def forward(ctx, s_qkv, t_qkv, B, N, hd_s, hd_t):
        L.require_device(s_qkv)
        dev = s_qkv.device
        Ds, Dt = s_qkv.shape[1] // 3, t_qkv.shape[1] // 3
        ctx.fused = relation_fused_selected(s_qkv, t_qkv, B, N)
        if ctx.fused:
            losses = torch.empty(3, dtype=F32, device=dev)
            stats = torch.empty((3, 3, B * N), dtype=F32, device=dev)      # lse_t, lse_s, row_kl: dead after the reduce
            S = torch.empty((3, B, 208, 224), dtype=BF16, device=dev)
            call("devit_relation_fused_fwd", ptr(s_qkv), ptr(t_qkv), B, N, Ds, Dt, s_qkv.stride(0), t_qkv.stride(0), hd_t, hd_s,
                 int(t_qkv.dtype == F16), ptr(stats[0]), ptr(stats[1]), ptr(stats[2]), ptr(S), ptr(losses), stream_ptr())
            ctx.S, ctx.s_qkv = S, s_qkv
            ctx.meta = (B, N, hd_s, hd_t, Ds)
            return losses
        assert s_qkv.shape[0] >= (B - 1) * N + 256 and t_qkv.shape[0] >= (B - 1) * N + 256, "packed qkv needs pad rows"
        losses = torch.empty(3, dtype=F32, device=dev)
        grams, stats = [], []
        for j in range(3):
            gt = torch.empty((B, 256, 256), dtype=F32, device=dev)
            gs = torch.empty((B, 256, 256), dtype=F32, device=dev)
            for buf, Dm, out in ((t_qkv, Dt, gt), (s_qkv, Ds, gs)):
                f = buf[:, j * Dm:]
                gemm(f, 3 * Dm, 0, f, 3 * Dm, 0, 256, 256, Dm, kind=L.EPI_STORE_F32, out=out, ldc=256, batch=B,
                     a_bs=N * 3 * Dm, b_bs=N * 3 * Dm, out_bs=256 * 256, dtype16=int(buf.dtype == F16))
            lse_t = torch.empty((B, N), dtype=F32, device=dev)
            lse_s = torch.empty((B, N), dtype=F32, device=dev)
            row_kl = torch.empty((B, N), dtype=F32, device=dev)
            call("devit_relation_stats", ptr(gt), ptr(gs), B, N, 256, hd_t, hd_s, ptr(lse_t), ptr(lse_s), ptr(row_kl),
                 ptr(losses[j:]), stream_ptr())
            grams.append((gt, gs))
            stats.append((lse_t, lse_s))
        ctx.grams, ctx.stats, ctx.s_qkv = grams, stats, s_qkv
        ctx.meta = (B, N, hd_s, hd_t, Ds)
        return losses

    @staticmethod
    def backward(ctx, g):
        B, N, hd_s, hd_t, Ds = ctx.meta
        s_qkv = ctx.s_qkv
        dev = s_qkv.device
        g = g.contiguous().float()
        d = torch.empty_like(s_qkv)       # rows < B*N are all written below (N rows per image x 3 components)
        if ctx.fused:
            call("devit_relation_fused_bwd", ptr(ctx.S), ptr(s_qkv), ptr(g), B, N, Ds, s_qkv.stride(0), ptr(d), d.stride(0), stream_ptr())
            ctx.S = None
            return d, None, None, None, None, None
        S = torch.empty((B, 256, 256), dtype=BF16, device=dev)
        for j in range(3):
            gt, gs = ctx.grams[j]
            lse_t, lse_s = ctx.stats[j]
            call("devit_relation_grad", ptr(gt), ptr(gs), ptr(lse_t), ptr(lse_s), ptr(g[j:]), B, N, 256, hd_t, hd_s,
                 ptr(S), 0, stream_ptr())
            f = s_qkv[:, j * Ds:]
            # dF[b] (rows < N) = S[b] @ F[b]   (F read k-major; rows >= N of S are zero)
            gemm(S, 256, 0, f, 3 * Ds, 1, 256, Ds, 256, kind=L.EPI_STORE_BF16, out=d[:, j * Ds:], ldc=3 * Ds, batch=B,
                 a_bs=256 * 256, b_bs=N * 3 * Ds, out_bs=N * 3 * Ds, m_valid=N)
        ctx.grams = ctx.stats = None
        return d, None, None, None, None, None


# ---- cal_qkv_loss / cal_qkv_loss2 / soft_cross_entropy (utils/losses.py:37-41, 247-292) -- csrc/qkvce.hip ----
QKV_LAYOUTS = {"view": 0, "tokens": 1}


class QkvPairLossFn(torch.autograd.Function):
    """One layer pair of cal_qkv_loss (cross=False: the three pairs (i, i)) or cal_qkv_loss2 (cross=True: all nine ordered pairs) on PACKED qkv
    buffers: the mean soft cross-entropy of the pairs' Grams X_i X_j^T / 8, divided by `layers`.  s_qkv: bf16 [>= B N rows, 3 Ds], t_qkv bf16 or
    f16 likewise with Dt; heads are 64 wide.  layout "view": rows as the reference's `.view(B, N, H * 64)` of [B, H, N, 64] reinterprets them;
    "tokens": head-concatenated token rows.  Returns an fp32 scalar; the gradient goes to the student buffer.  The context keeps the bf16 S of the
    three or nine slots and nothing else of the forward."""

    @staticmethod
    def forward(ctx, s_qkv, t_qkv, B, N, cross, layout, layers):
        L.require_device(s_qkv)
        if layout not in QKV_LAYOUTS:
            raise ValueError(f"layout must be one of {sorted(QKV_LAYOUTS)}, got {layout!r}")
        if s_qkv.dtype == F32:
            raise NotImplementedError('cal_qkv_loss / cal_qkv_loss2: a precision="f32" student (an fp32 packed qkv buffer) is not built: these '
                                      'losses run on the 16-bit MFMA path only (DESIGN.md)')
        if s_qkv.dtype != BF16 or t_qkv.dtype not in (BF16, F16) or s_qkv.dim() != 2 or t_qkv.dim() != 2 or s_qkv.stride(1) != 1 \
                or t_qkv.stride(1) != 1 or s_qkv.shape[0] < B * N or t_qkv.shape[0] < B * N or s_qkv.shape[1] % 3 or t_qkv.shape[1] % 3:
            raise L.DevitError(f"QkvPairLossFn: a bf16 student and a bf16 / f16 teacher packed [>= B N, 3 D] buffer, got {tuple(s_qkv.shape)} "
                               f"{s_qkv.dtype} and {tuple(t_qkv.shape)} {t_qkv.dtype} for B={B} N={N}")
        dev = s_qkv.device
        Ds, Dt = s_qkv.shape[1] // 3, t_qkv.shape[1] // 3
        P = 9 if cross else 3
        loss = torch.empty(1, dtype=F32, device=dev)
        terms = torch.empty((P, B * N), dtype=F32, device=dev)            # dead after the reduce
        S = torch.empty((P, B, 208, 224), dtype=BF16, device=dev)
        call("devit_qkv_pair_fwd", ptr(s_qkv), ptr(t_qkv), B, N, Ds, Dt, s_qkv.stride(0), t_qkv.stride(0), 64, 64, int(t_qkv.dtype == F16),
             int(bool(cross)), QKV_LAYOUTS[layout], int(layers), ptr(terms), ptr(S), ptr(loss), stream_ptr())
        ctx.S, ctx.s_qkv = S, s_qkv
        ctx.meta = (B, N, Ds, int(bool(cross)), QKV_LAYOUTS[layout])
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        B, N, Ds, cross, layout = ctx.meta
        s_qkv = ctx.s_qkv
        g = g.contiguous().float()
        d = torch.empty_like(s_qkv)       # rows < B*N are all written below (every 64-wide chunk of the three components has one writer)
        call("devit_qkv_pair_bwd", ptr(ctx.S), ptr(s_qkv), ptr(g), B, N, Ds, s_qkv.stride(0), 64, cross, layout, ptr(d), d.stride(0),
             stream_ptr())
        ctx.S = None
        return d, None, None, None, None, None, None


class SoftCrossEntropyFn(torch.autograd.Function):
    """utils/losses.py:37-41 on fp32 rows: mean over the rows of -sum softmax(targets) log_softmax(predicts); the gradient goes to predicts."""

    @staticmethod
    def forward(ctx, predicts, targets):
        L.require_device(predicts)
        if predicts.shape != targets.shape or predicts.dim() < 1 or predicts.numel() == 0:
            raise L.DevitError(f"soft_cross_entropy: predicts {tuple(predicts.shape)} and targets {tuple(targets.shape)} must agree and be non-empty")
        C_ = predicts.shape[-1]
        p = predicts.detach().reshape(-1, C_).contiguous().float()
        t = targets.detach().reshape(-1, C_).contiguous().float()
        R = p.shape[0]
        row_loss = torch.empty(R, dtype=F32, device=p.device)
        loss = torch.empty(1, dtype=F32, device=p.device)
        call("devit_soft_ce_rows_fwd", ptr(p), ptr(t), R, C_, ptr(row_loss), ptr(loss), stream_ptr())
        ctx.keep, ctx.shape, ctx.dtype = (p, t), predicts.shape, predicts.dtype
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        p, t = ctx.keep
        ctx.keep = None
        dp = torch.empty_like(p)
        call("devit_soft_ce_rows_bwd", ptr(p), ptr(t), ptr(g.contiguous().float()), p.shape[0], p.shape[1], ptr(dp), stream_ptr())
        return dp.reshape(ctx.shape).to(ctx.dtype), None


# ---- hidden-state relation loss (utils/losses.py:295-304, cal_hid_relation_loss) -- csrc/hid.hip ----
HID_EPS = 1e-12       # torch.nn.functional.normalize's default eps


def hid_normalize(h, exact=False):
    """fp32 [B, N, D] -> (h^ = h / max(|h|, 1e-12) packed as bf16 (exact: fp32) [pad_rows(B N) + qkv_pad_rows(N), ld], ld = D rounded up to 128, with zero
    pad columns and zero rows behind B N: what the 256-row Gram windows and the 128-wide GEMM tiles read; inv fp32 [B N] = 1 / max(|h|, 1e-12))."""
    L.require_device(h)
    if h.dim() != 3:
        raise L.DevitError(f"cal_hid_relation_loss: hidden states are [B, N, D], got {tuple(h.shape)}")
    B, N, D = h.shape
    h = h.contiguous().float()
    if h.data_ptr() % 16:
        h = h.clone()
    ld = (D + 127) // 128 * 128
    rows = pad_rows(B * N) + qkv_pad_rows(N)
    hn = torch.empty((rows, ld), dtype=F32 if exact else BF16, device=h.device)
    inv = torch.empty(B * N, dtype=F32, device=h.device)
    call("devit_hid_normalize", ptr(h), ptr(hn), ptr(inv), B, N, D, ld, rows, int(exact), HID_EPS, stream_ptr())
    return hn, inv


def hid_gram(hn, B, N, D, exact=False):
    """Per-image Grams h^ h^T of a hid_normalize buffer as padded fp32 [B, 256, 256] (entries outside N x N: the neighbouring image's rows, or,
    in exact mode, zeros: nobody reads them)."""
    ld = hn.shape[1]
    if exact:
        from .ops_f32 import sgemm
        g = torch.zeros((B, 256, 256), dtype=F32, device=hn.device)
        sgemm(hn, ld, 1, hn, ld, 1, N, N, D, out=g, ldc=256, batch=B, a_bo=N * ld, b_bo=N * ld, c_bo=65536)
        return g
    g = torch.empty((B, 256, 256), dtype=F32, device=hn.device)
    gemm(hn, ld, 0, hn, ld, 0, 256, 256, ld, kind=L.EPI_STORE_F32, out=g, ldc=256, batch=B, a_bs=N * ld, b_bs=N * ld, out_bs=65536)
    return g


def hid_stats(gs, gt, B, N, layers=1):
    """fp32 [1]: sum (G_s - G_t)^2 / (B N^2 layers)"""
    row_sq = torch.empty(B * N, dtype=F32, device=gs.device)
    loss = torch.empty(1, dtype=F32, device=gs.device)
    call("devit_hid_stats", ptr(gs), ptr(gt), B, N, 256, layers, ptr(row_sq), ptr(loss), stream_ptr())
    return loss


def hid_grad(gs, gt, upstream, B, N, layers=1, exact=False):
    """S = (4 upstream / (B N^2 layers)) (G_s - G_t): bf16 (exact: fp32) [B, 256, 256], zero outside N x N; upstream: fp32 device scalar or None (1)"""
    S = torch.empty((B, 256, 256), dtype=F32 if exact else BF16, device=gs.device)
    call("devit_hid_grad", ptr(gs), ptr(gt), ptr(upstream), B, N, 256, layers, ptr(S), int(exact), stream_ptr())
    return S


def hid_dhn(S, hn, B, N, D, exact=False):
    """dh^ = S h^ per image: fp32 [B N, ld] (fp32 accumulation over the 256-wide window; S is zero there outside N x N)"""
    ld = hn.shape[1]
    if exact:
        from .ops_f32 import sgemm
        dhn = torch.zeros((B * N, ld), dtype=F32, device=hn.device)
        sgemm(S, 256, 1, hn, 1, ld, N, D, N, out=dhn, ldc=ld, batch=B, a_bo=65536, b_bo=N * ld, c_bo=N * ld)
        return dhn
    dhn = torch.empty((B * N, ld), dtype=F32, device=hn.device)
    gemm(S, 256, 0, hn, ld, 1, 256, ld, 256, kind=L.EPI_STORE_F32, out=dhn, ldc=ld, batch=B, a_bs=65536, b_bs=N * ld, out_bs=N * ld,
         m_valid=N)
    return dhn


def hid_normalize_bwd(hn, dhn, inv, B, N, D):
    """dh = inv (dh^ - h^ (h^ . dh^)): fp32 [B, N, D]"""
    dh = torch.empty((B, N, D), dtype=F32, device=hn.device)
    call("devit_hid_normalize_bwd", ptr(hn), ptr(dhn), ptr(inv), ptr(dh), B, N, D, hn.shape[1], int(hn.dtype == F32), stream_ptr())
    return dh


class HidRelationLossFn(torch.autograd.Function):
    """One (student, teacher) pair of cal_hid_relation_loss: mean((G_s - G_t)^2) / layers with G = h^ h^T per image of the row-normalised
    hidden states.  s: fp32 [B, N, Ds], t: fp32 [B, N, Dt]; the gradient goes to the student.  exact: fp32 h^, Grams and products
    (devit_gemm_f32) instead of one bf16 rounding of h^ and of S."""

    @staticmethod
    def forward(ctx, s, t, layers, exact):
        B, N, Ds = s.shape
        if tuple(t.shape[:2]) != (B, N):
            raise L.DevitError(f"cal_hid_relation_loss: student {tuple(s.shape)} and teacher {tuple(t.shape)} differ in batch or tokens")
        hs, inv_s = hid_normalize(s, exact)
        ht, _ = hid_normalize(t, exact)
        gs, gt = hid_gram(hs, B, N, Ds, exact), hid_gram(ht, B, N, t.shape[2], exact)
        ctx.keep, ctx.meta = (hs, inv_s, gs, gt), (B, N, Ds, layers, exact)
        return hid_stats(gs, gt, B, N, layers)[0]

    @staticmethod
    def backward(ctx, g):
        hs, inv_s, gs, gt = ctx.keep
        B, N, Ds, layers, exact = ctx.meta
        ctx.keep = None
        S = hid_grad(gs, gt, g.contiguous().float(), B, N, layers, exact)
        return hid_normalize_bwd(hs, hid_dhn(S, hs, B, N, Ds, exact), inv_s, B, N, Ds), None, None, None
