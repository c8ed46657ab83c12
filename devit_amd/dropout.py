"""nn.Dropout with p > 0 on the HIP path: the host side of the ONE mask definition (include/devit_hip.h, "Dropout"; csrc/dropout.h) and tensor-level
wrappers over its entry points.  The mask is a function of (seed, site, block, element index) -- Philox4x32-10 -- and is never stored."""
import math

import torch

from . import _lib as L
from ._lib import ptr, stream_ptr

BF16, F32 = torch.bfloat16, torch.float32
SITES = {"pos_drop": L.DROP_POS, "attn_drop": L.DROP_ATTN, "proj_drop": L.DROP_PROJ, "mlp_hidden": L.DROP_HIDDEN, "mlp_out": L.DROP_FC2}


def check_p(p, what="dropout p"):
    """p as a float in [0, 1) -- p == 1 has no finite 1 / (1 - p) -- else ValueError."""
    p = float(p)
    if not (0.0 <= p < 1.0):          # (also refuses NaN)
        raise ValueError(f"{what} must be in [0, 1), got {p}")
    return p


def threshold(p):
    """(thr, scale_keep) of a drop probability: an element is kept iff its 32-bit Philox word >= thr = min(floor(p 2^32), 2^32 - 1) (double
    precision, as the header states it), and kept values are multiplied by float32(1 / (1 - p))."""
    p = check_p(p)
    return min(int(math.floor(p * 4294967296.0)), 4294967295), 1.0 / (1.0 - p)


def ceil4(n):
    return (n + 3) & ~3


def keep_mask(seed, site, block, p, rows, cols, pitch=None, device="cuda"):
    """The keep bytes ([rows][cols] uint8, 1 = kept) of a site as the kernels generate them (devit_dropout_mask: debug / tests)."""
    thr, _ = threshold(p)
    keep = torch.empty((rows, cols), dtype=torch.uint8, device=device)
    L.require_device(keep)
    L.call("devit_dropout_mask", seed, site, block, thr, rows, cols, ceil4(cols) if pitch is None else pitch, ptr(keep), stream_ptr())
    return keep


def apply_(x, rows, seed, site, block, p, colsum=None, pitch=None):
    """In place on rows [0, rows) of a contiguous 2-D bf16 / fp32 buffer: x = keep * x / (1 - p); colsum (fp32 [cols]) += column sums of the result."""
    assert x.dim() == 2 and x.is_contiguous() and x.dtype in (BF16, F32) and rows <= x.shape[0]
    L.require_device(x)
    thr, s = threshold(p)
    cols = x.shape[1]
    L.call("devit_dropout_apply", ptr(x), 1 if x.dtype == F32 else 0, rows, cols, cols, cols if pitch is None else pitch, seed, site, block,
           thr, s, ptr(colsum), stream_ptr())
    return x


def residual(x, y, rowscale, rows_per_scale, seed, site, block, p, out=None):
    """out = x + rowscale[m // rows_per_scale] * keep * y / (1 - p) on fp32 [rows][cols] (out: a new tensor, or any of the same shape, x included)."""
    assert x.dim() == 2 and x.shape == y.shape and x.dtype == F32 and y.dtype == F32 and x.is_contiguous() and y.is_contiguous()
    L.require_device(x)
    thr, s = threshold(p)
    out = torch.empty_like(x) if out is None else out
    L.call("devit_dropout_residual", ptr(x), ptr(y), ptr(out), ptr(rowscale), rows_per_scale, x.shape[0], x.shape[1], seed, site, block,
           thr, s, stream_ptr())
    return out
