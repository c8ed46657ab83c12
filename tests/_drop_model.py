"""Float64 statements, bounds, fp32 emulations and planted bugs for the three kernels of csrc/dropout.hip (devit_dropout_mask / _apply /
_residual), and the case table the CPU test (tests/test_dropout_model.py) and the GPU tests (tests/test_gpu_dropout.py) share.

The statements are written from the header's text (include/devit_hip.h, "Dropout"; csrc/dropout.h): element (r, c) of a logical tensor of
row pitch `pitch` has index e = r * pitch + c, its keep bit is word e & 3 of Philox4x32-10 at counter (e >> 2 low, e >> 2 high, site, block)
compared with thr.  Masks come from tests/_philox.py only, one element at a time; nothing here reads devit_dropout_mask.

    mask      keep[r][c], bit for bit.
    apply     stored = bf16(fp32(x) * s) (bf16 buffers) or fp32(x * s) where kept, +0 where dropped: bit for bit.  Columns [cols, ld) and
              whatever lies behind the buffer keep their bits.
              colsum[c] = colsum0[c] + sum_r stored[r][c].  The kernel adds in fp32: a lane walks rows r0, r0 + 4 gy, ... (its strip, at
              most ceil(rows / (4 gy)) adds), thread row 0 adds the RY = 4 partial sums of its workgroup (3 adds) and the gy workgroups of
              a column add theirs to colsum with one atomicAdd each, in any order (gy adds).  Every add rounds to nearest: relative error
              2^-24 of a partial sum that is at most |colsum0| + sum |stored| in magnitude, so
                  |got - colsum| <= (strip + 3 + gy) 2^-24 (|colsum0[c]| + sum_r |stored[r][c]|)          first order, no free factor
              with gy from row_grid(): min(ceil(rows / 4), 256 / gx) workgroups of rows when colsum is given, gx = ceil(lanes / 64).
    residual  out = x + rs y s where kept, with rs = rowscale[r / rows_per_scale] or 1; the kernel rounds twice (the product y * s and
              the fmaf):  |out - (x + rs y s)| <= 2^-24 (|rs y s| + |out|).  Where the element is dropped or rs == 0, out has x's bits.

emulate_*() restate the kernels' index arithmetic group by group (one Philox call per four columns, as a lane makes it) in numpy / fp32
torch, and take `mutate`: one of MUTATIONS, each a wrong index a kernel of this shape could have.  judge_*() return, per named output, the
worst |err| / bound; an output the model states bit for bit gives 0.0 or inf."""
import functools
import math

import numpy as np
import torch

import _philox as PH

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
U24 = 2.0 ** -24
CX, RY = 64, 4                      # a workgroup of dropout.hip: 64 lanes of 16 bytes along a row, 4 rows
MASK_GRID, MASK_WG = 4096, 256      # devit_dropout_mask: at most 4096 workgroups of 256 lanes, one column group per lane and trip
SEED = 20240807
SEED64 = (0x9E3779B9 << 32) | 0x12345678
MUTATIONS = ("c0_missing", "ld_for_pitch", "rowscale_mod", "high_word_dropped", "second_half_e0")


def ceil4(n):
    return (n + 3) & ~3


# ------------------------------------------------------------------------------------------ the case table
def _m(name, rows, cols, pitch, site=3, block=5, p=0.1, seed=SEED):
    return dict(kernel="mask", name=name, rows=rows, cols=cols, pitch=pitch, site=site, block=block, p=p, seed=seed)


def _a(name, dtype, rows, cols, ld=None, pitch=None, colsum=True, site=3, block=5, p=0.1):
    return dict(kernel="apply", name=name, dtype=dtype, rows=rows, cols=cols, ld=cols if ld is None else ld,
                pitch=cols if pitch is None else pitch, colsum=colsum, site=site, block=block, p=p, seed=SEED)


def _r(name, rows, cols, rps, rowscale, in_place, site=2, block=7, p=0.1):
    return dict(kernel="residual", name=name, rows=rows, cols=cols, rps=rps, rowscale=rowscale, in_place=in_place, site=site, block=block,
                p=p, seed=SEED)


MASK_CASES = [
    _m("c1-tight", 5, 9, 12, site=0, block=0), _m("c1-wide", 5, 9, 20, p=0.5),
    _m("c2-tight", 5, 10, 12, site=4, block=11, p=0.5), _m("c2-wide", 5, 10, 24, site=0, block=11),
    _m("c3-tight", 5, 11, 12, site=1, block=0), _m("c3-wide", 5, 11, 16, site=4, block=1, p=0.5),
    _m("hi-2p34", 3, 10, 2 ** 34, p=0.5), _m("hi-2p34+4", 3, 10, 2 ** 34 + 4),
    _m("stride", 1025, 4097, 4100, site=2, block=3),
    _m("seed64", 7, 10, 12, seed=SEED64, p=0.25),
]
APPLY_CASES = [
    _a("bf16-1029x520-sum", BF16, 1029, 520), _a("f32-1029x260-sum", F32, 1029, 260, p=0.5),
    _a("bf16-4101x520", BF16, 4101, 520, colsum=False, p=0.5),
    _a("bf16-ld", BF16, 37, 520, ld=544, pitch=1040, site=4, block=0), _a("f32-ld", F32, 37, 260, ld=272, pitch=520, site=0, block=1, p=0.5),
    _a("bf16-hi", BF16, 3, 520, pitch=2 ** 34, p=0.5), _a("f32-hi", F32, 3, 260, pitch=2 ** 34 + 4),
]
RESIDUAL_CASES = [
    _r("4101x260-rps3", 4101, 260, 3, "zeros", False), _r("4101x260-rps198", 4101, 260, 198, "zeros", True, p=0.5),
    _r("37x260-null", 37, 260, 0, None, False, p=0.5), _r("37x260-null-inplace", 37, 260, 0, None, True, site=4, block=0),
]
CASES = {c["kernel"] + "/" + c["name"]: c for c in MASK_CASES + APPLY_CASES + RESIDUAL_CASES}


def thr_s(p):
    """(thr, the fp32 value of 1 / (1 - p)) as the header states them"""
    return PH.threshold(p), float(np.float32(1.0 / (1.0 - p)))


# ------------------------------------------------------------------------------------------ grids (dropout.hip: row_grid and the mask launch)
def row_grid(rows, lanes_x, max_groups=2048):
    gx = (lanes_x + CX - 1) // CX
    gy = (rows + RY - 1) // RY
    cap = max(max_groups // gx, 1)
    return gx, max(min(gy, cap), 1)


def grid(c):
    """-> dict: gx, gy, trips (row-loop trips of the busiest lane; for the mask, loop trips of lane 0)"""
    if c["kernel"] == "mask":
        total = c["rows"] * ((c["cols"] + 3) // 4)
        g = min((total + MASK_WG - 1) // MASK_WG, MASK_GRID)
        return dict(gx=g, gy=1, trips=(total + g * MASK_WG - 1) // (g * MASK_WG))
    if c["kernel"] == "apply":
        V = 4 if c["dtype"] == F32 else 8
        gx, gy = row_grid(c["rows"], c["cols"] // V, 256 if c["colsum"] else 2048)
    else:
        gx, gy = row_grid(c["rows"], c["cols"] // 4)
    return dict(gx=gx, gy=gy, trips=(c["rows"] + gy * RY - 1) // (gy * RY))


def high_word_max(c):
    """the largest high counter word (group >> 32) any element of the case has"""
    return ((c["rows"] - 1) * c["pitch"] + c["cols"] - 1) >> 34


# ------------------------------------------------------------------------------------------ inputs and statements
@functools.lru_cache(maxsize=None)
def _keep(seed, site, block, thr, rows, cols, pitch):
    return torch.from_numpy(PH.keep_mask(seed, site, block, thr, rows, cols, pitch))


def keep_of(c, pitch=None):
    """bool [rows][cols] from the numpy mirror (cached: the CPU and GPU tests of one process share it; treat it as read-only)"""
    return _keep(c["seed"], c["site"], c["block"], thr_s(c["p"])[0], c["rows"], c["cols"], c.get("pitch", c["cols"]) if pitch is None else pitch)


def inputs(c):
    """CPU tensors of the case, seeded by its name.  apply: x [rows][ld], colsum0 [cols]; residual: x, y [rows][cols], rowscale or None"""
    gen = torch.Generator(device="cpu").manual_seed(sum(ord(ch) * (i + 1) for i, ch in enumerate(c["name"])))
    if c["kernel"] == "apply":
        return dict(x=torch.randn((c["rows"], c["ld"]), generator=gen).to(c["dtype"]), colsum0=torch.randn(c["cols"], generator=gen))
    x, y = torch.randn((c["rows"], c["cols"]), generator=gen), torch.randn((c["rows"], c["cols"]), generator=gen)
    rs = None
    if c["rowscale"] == "zeros":           # DropPath: a fifth of the groups off, the others 1 / 0.8
        n = (c["rows"] + c["rps"] - 1) // c["rps"]
        rs = (torch.rand(n, generator=gen) > 0.2).float().div(0.8)
        assert 0 < int((rs == 0).sum()) < n
    return dict(x=x, y=y, rowscale=rs)


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


def apply_statement(c, inp, keep=None):
    """-> stored [rows][cols] in the buffer's type (bit exact), colsum float64 [cols], its bound [cols]"""
    keep = keep_of(c) if keep is None else keep
    s = torch.tensor(thr_s(c["p"])[1], dtype=F32)
    x = inp["x"][:, :c["cols"]]
    stored = torch.where(keep, (x.to(F32) * s).to(c["dtype"]), torch.zeros((), dtype=c["dtype"]))
    g = grid(c)
    adds = g["trips"] + (RY - 1) + g["gy"]
    colsum = inp["colsum0"].to(F64) + stored.to(F64).sum(0)
    bound = adds * U24 * (inp["colsum0"].to(F64).abs() + stored.to(F64).abs().sum(0))
    return stored, colsum, bound


def residual_statement(c, inp, keep=None):
    """-> want float64 [rows][cols], the scaled branch rs y s (float64), exact (bool: out must have x's bits)"""
    keep = keep_of(c) if keep is None else keep
    s = thr_s(c["p"])[1]
    rows = c["rows"]
    rs = torch.ones(rows, dtype=F64) if inp["rowscale"] is None else inp["rowscale"].to(F64)[torch.arange(rows) // c["rps"]]
    branch = rs[:, None] * inp["y"].to(F64) * s
    want = inp["x"].to(F64) + torch.where(keep, branch, torch.zeros((), dtype=F64))
    return want, branch, ~keep | (rs[:, None] == 0)


# ------------------------------------------------------------------------------------------ judges: output name -> worst ratio
def _exact(got, want):
    return 0.0 if got.shape == want.shape and torch.equal(bits(got), bits(want)) else math.inf


def _ratio(err, bound):
    rt = torch.where(err == 0, torch.zeros_like(err), err / bound)
    rt = torch.where(torch.isfinite(err), rt, torch.full_like(rt, math.inf))
    return float(rt.max()) if rt.numel() else 0.0


def judge_mask(c, got):
    """got: uint8 / bool [rows][cols] on the CPU"""
    return dict(keep=0.0 if torch.equal(got.bool(), keep_of(c)) and (got.dtype == torch.bool or int(got.max()) <= 1) else math.inf)


def judge_apply(c, inp, x_after, colsum_after):
    """x_after [rows][ld] (CPU, the buffer's type), colsum_after fp32 [cols] or None -> x (bit exact), pad (columns [cols, ld) untouched),
    colsum (ratio against the bound)"""
    stored, colsum, bound = apply_statement(c, inp)
    cols = c["cols"]
    res = dict(x=_exact(x_after[:, :cols], stored), pad=_exact(x_after[:, cols:], inp["x"][:, cols:]))
    if c["colsum"]:
        res["colsum"] = _ratio((colsum_after.to(F64) - colsum).abs(), bound)
    return res


def judge_residual(c, inp, out):
    """out fp32 [rows][cols] on the CPU -> exact (x's bits where dropped or rowscale == 0), kept (ratio)"""
    want, branch, exact = residual_statement(c, inp)
    o64 = out.to(F64)
    kept = ~exact
    err = (o64 - want).abs()
    bound = U24 * (branch.abs() + o64.abs())
    return dict(exact=_exact(out[exact], inp["x"][exact]), kept=_ratio(err[kept], bound[kept]))


# ------------------------------------------------------------------------------------------ emulations: the kernels' index arithmetic
def _words(c, g):
    """four uint32 arrays: the Philox words of the column groups g (uint64 array), as drop_words() forms the counter"""
    seed = c["seed"]
    return PH.philox4x32_10((g & PH.MASK, g >> np.uint64(32), np.uint64(c["site"]), np.uint64(c["block"])), (seed & 0xFFFFFFFF, seed >> 32))


def _lane_keep(c, lanes_cols, row_pitch, mutate, v=4):
    """bool [rows][len(lanes_cols) * v]: every lane's c0 in `lanes_cols`, v elements per lane (8: two Philox calls, e0 and e0 + 4)"""
    thr = np.uint32(thr_s(c["p"])[0])
    r = np.arange(c["rows"], dtype=np.uint64)[:, None]
    c0 = np.asarray(lanes_cols, dtype=np.uint64)[None, :]
    e0 = r * np.uint64(row_pitch) + (c0 * np.uint64(0) if mutate == "c0_missing" else c0)
    halves = []
    for h in range(v // 4):
        e = e0 + np.uint64(0 if mutate == "second_half_e0" else 4 * h)
        g = e >> np.uint64(2)
        if mutate == "high_word_dropped":
            g = g & PH.MASK
        halves.append(np.stack(_words(c, g), axis=-1) >= thr)          # [rows][lanes][4]
    return np.concatenate(halves, axis=-1).reshape(c["rows"], -1)


def emulate_mask(c, mutate=None):
    cols = c["cols"]
    return torch.from_numpy(_lane_keep(c, np.arange((cols + 3) // 4) * 4, c["pitch"], mutate)[:, :cols].copy())


def emulate_apply(c, inp, mutate=None):
    """-> (x_after [rows][ld], colsum_after fp32 or None): fp32 arithmetic in the kernel's order, workgroups' atomics in index order"""
    V = 4 if c["dtype"] == F32 else 8
    rows, cols = c["rows"], c["cols"]
    keep = torch.from_numpy(_lane_keep(c, np.arange(cols // V) * V, c["ld"] if mutate == "ld_for_pitch" else c["pitch"], mutate, V))
    s = torch.tensor(thr_s(c["p"])[1], dtype=F32)
    x_after = inp["x"].clone()
    stored = torch.where(keep, (inp["x"][:, :cols].to(F32) * s).to(c["dtype"]), torch.zeros((), dtype=c["dtype"]))
    x_after[:, :cols] = stored
    if not c["colsum"]:
        return x_after, None
    g = grid(c)
    gy, trips = g["gy"], g["trips"]
    padded = torch.zeros((trips * gy * RY, cols), dtype=F32)
    padded[:rows] = stored.to(F32)
    strips = padded.view(trips, gy, RY, cols)                  # row = (trip gy + by) 4 + ty
    acc = torch.zeros((gy, RY, cols), dtype=F32)
    for t in range(trips):
        acc = acc + strips[t]
    part = acc[:, 0]
    for y in range(1, RY):
        part = part + acc[:, y]
    colsum = inp["colsum0"].clone()
    for by in range(gy):
        colsum = colsum + part[by]
    return x_after, colsum


def emulate_residual(c, inp, mutate=None):
    """fp32: t = y * s rounded, out = fmaf(rs, t, x) (the product rs t is exact in float64; its sum with x is rounded there and again to
    fp32, which differs from the one rounding of an fma only on a tie of the second rounding)"""
    rows, cols = c["rows"], c["cols"]
    keep = torch.from_numpy(_lane_keep(c, np.arange(cols // 4) * 4, cols, mutate))
    s = torch.tensor(thr_s(c["p"])[1], dtype=F32)
    r = torch.arange(rows)
    if inp["rowscale"] is None:
        rs = torch.ones(rows, dtype=F32)
    else:
        rs = inp["rowscale"][(r % c["rps"]) if mutate == "rowscale_mod" else (r // c["rps"])]
    t = inp["y"] * s
    fused = (rs.to(F64)[:, None] * t.to(F64) + inp["x"].to(F64)).to(F32)
    return torch.where(keep, fused, inp["x"])


# mutation -> (case, outputs it must break (ratio >= 1), outputs it must leave below 1)
PLANTED = {
    "c0_missing": [("mask/c1-wide", ("keep",), ()), ("apply/f32-1029x260-sum", ("x", "colsum"), ("pad",)),
                   ("residual/37x260-null", ("kept", "exact"), ())],
    "ld_for_pitch": [("apply/bf16-ld", ("x", "colsum"), ("pad",)), ("apply/f32-ld", ("x", "colsum"), ("pad",))],
    "rowscale_mod": [("residual/4101x260-rps3", ("kept", "exact"), ())],       # (at 198 rows per scale r % 198 would read past rowscale)
    "high_word_dropped": [("mask/hi-2p34", ("keep",), ()), ("mask/hi-2p34+4", ("keep",), ()), ("apply/bf16-hi", ("x", "colsum"), ("pad",)),
                          ("apply/f32-hi", ("x", "colsum"), ("pad",))],
    "second_half_e0": [("apply/bf16-1029x520-sum", ("x", "colsum"), ("pad",)), ("apply/bf16-4101x520", ("x",), ("pad",))],
}


def run_emulation(c, mutate=None):
    """-> judge's dict for the emulation of case c"""
    if c["kernel"] == "mask":
        return judge_mask(c, emulate_mask(c, mutate))
    inp = inputs(c)
    if c["kernel"] == "apply":
        return judge_apply(c, inp, *emulate_apply(c, inp, mutate))
    return judge_residual(c, inp, emulate_residual(c, inp, mutate))
