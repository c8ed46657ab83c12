"""Float64 statements, first-order elementwise error bounds, an fp32 emulation with planted bugs, ONE case table and seeded inputs for the 16-bit MFMA
GEMM family behind devit_gemm_bf16 and devit_wgrad_grouped (csrc/gemm.hip, gemm_tile.h, gemm_device.h, gemm4.hip, gemmfr.hip, wgradfr.hip).  Plain
torch; it runs wherever its inputs live.  Shared by tests/test_gemm_model.py (the model itself under test, no GPU) and tests/test_gpu_gemm.py (the
kernels under test), which therefore see the same cases and the same inputs.  ratio, stored16, gen, U, H_BF16, H_F16 are those of _tail_model.

What a call reads and writes is stated on the PHYSICAL buffers: an operand is (buffer, element offset, ld, kmajor, row_group, row_skip, batch stride)
exactly as devit_operand describes it, and logical() gathers the [batch][rows][K] matrix the header's words define from it.  Everything of a buffer
that the description does not name holds NaN (inputs) or a sentinel that must come back bit for bit (outputs): verdict() checks both.

Convention of every bound (no factor on top, nothing fitted to what the kernels deliver):
  accumulator   the product of two 16-bit values is exact in fp32; the MFMA sums are taken as in _attn_model: E32 = 2^-23 per addition.
                E_acc = E32 (K + s) sum_k |a_k| |b_k|, s = the further fp32 additions counted from the source: the split-K atomics and the value
                the accumulator held (gemm_tile.h:385: one unsafeAtomicAdd per slice), the row-sum folds (gemm_tile.h:397-398: 2) and the atomics
                of the (m-tile, slice, n-tile) shares of a row sum (gemm_tile.h:305,400: split_k * tiles_n).
  epilogue      u = 2^-24 per rounding, counted from epilogue_direct / epilogue_f32_rows (gemm_device.h), each count names its lines below;
                v_exp / v_rcp cost 2 (the cost _tail_model gives a device transcendental).
  16-bit stores stored16(): 2^-8 |ref| (bf16) or 2^-11 |ref| + 2^-25 (f16) on top of the carried fp32 error.
  GELU / dGELU  the fitted form's own documented error, 2.6e-5 and 1.2e-4 absolute (devit_common.h:78; tests/test_gemm_model.py verifies both against
                the erf form), plus E_pre propagated through |gelu'| to first order, plus the fitted form's fp32 arithmetic.
                The GELU is applied to the fp32 acc + bias (gemm_device.h:360-364: x[e] is packed into the saved pre-activation and, unrounded, fed
                to gelu_fwd), NOT to the rounded pre-activation that is stored beside it; the dGELU reads the stored 16-bit value (:367).

emulate() redoes the operations in fp32 torch in an order of its own (K in blocks of 64, every slice summed apart) with the kernel's fitted GELU.
It must stay at ratio <= 0.5 (16-bit stores: < 1, as in _tail_model), and every planted bug (`mutate=`) must reach >= 1, or break torch.equal in an
exact-integer case, or change a sentinel, on a named output of a named case (tests/test_gemm_model.py holds the list)."""
import math
import os
import re

import torch

from _tail_model import BF16, F16, F32, F64, H_BF16, H_F16, U, gen, ratio, stored16   # noqa: F401  (re-exported to the two test files)

E32 = 2.0 ** -23          # per fp32 addition of an MFMA / atomic sum (_attn_model.E32)
SENT = -123.0             # exact in bf16, f16 and fp32
GUARD = 64
NAN = math.nan
PAD = 8                   # elements between the matrix and its leading dimension: ld = width + 8 everywhere

# devit_epilogue_kind, DEVIT_ROUTE_* (include/devit_hip.h)
STORE_BF16, GELU, RESIDUAL, PATCH, DGELU, ATOMIC, STORE_F32 = range(7)
KIND_NAMES = ("STORE_BF16", "GELU", "RESIDUAL", "PATCH", "DGELU", "ATOMIC", "STORE_F32")
TILE128, TILE256, FULL_ROW, GEMM4 = 1, 3, 4, 5
ROUTE_NAMES = {TILE128: "TILE128", TILE256: "TILE256", FULL_ROW: "FULL_ROW", GEMM4: "GEMM4"}
# the switches that put a case on its route (both are read per call); a route's other switch is unset.  DEVIT_GEMM_FORCE must be unset.
ROUTE_ENV = {TILE128: {}, TILE256: {"DEVIT_GEMM4": "0"}, GEMM4: {"DEVIT_GEMM4": "1"}, FULL_ROW: {"DEVIT_GEMMFR": "1"}}
ROUTE_SWITCHES = ("DEVIT_GEMM4", "DEVIT_GEMMFR")
OUT16 = (STORE_BF16, GELU, DGELU)          # kinds whose `out` is 16-bit

COLSCALES = (0.0, 1.0, 0.5, -1.5, 3.0)
ROWSCALES = (0.0, 1.0, 1.25, 1.0 / 0.9)

MUTATIONS = ("last_product_dropped", "bias_from_left_at_tile_edge", "colscale_on_saved_preactivation", "rowscale_tile_local",
             "m_valid_plus_one", "row_skip_without_plus_one", "patch_without_tok", "gelu_without_clamp", "f16_store_through_bf16",
             "split_slice_twice", "colsum_of_wrong_operand")


# ============================================================================================ the fitted GELU (devit_common.h)
def _gelu_constants():
    """GELU_C0..2 and the fit's documented errors, read from the header text of csrc/devit_common.h (not copied)"""
    here = os.path.dirname(os.path.abspath(__file__))
    src = open(os.path.join(here, "..", "devit_amd", "csrc", "devit_common.h")).read()
    m = re.search(r"GELU_C0 = ([-0-9.e]+)f, GELU_C1 = ([-0-9.e]+)f, GELU_C2 = ([-0-9.e]+)f;", src)
    d = re.search(r"\|gelu error\| <= ([0-9.e-]+), \|gelu' error\| <= ([0-9.e-]+)", src)
    clamp = re.search(r"fminf\(x \* x, ([0-9.]+)f\)", src)
    c = tuple(float(torch.tensor(float(v), dtype=F32)) for v in m.groups())     # the fp32 values the compiler sees
    return c, float(d.group(1)), float(d.group(2)), float(clamp.group(1))


GELU_C, GELU_FIT_ERR, DGELU_FIT_ERR, GELU_CLAMP = _gelu_constants()


def gelu_exact(x):
    """the erf form (nn.GELU, models/de_vit.py:36) in the dtype of x (float64 in every reference)"""
    return 0.5 * x * (1 + torch.erf(x * math.sqrt(0.5)))


def dgelu_exact(x):
    return 0.5 * (1 + torch.erf(x * math.sqrt(0.5))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi)


def _fit_parts(x, clamp=True):
    """x2, u = x P(x2), s = sigmoid(u), u' = c0 + 3 c1 x2 + 5 c2 x2^2 of gelu_fwd<false> / gelu_bwd<false>, in the dtype of x"""
    c0, c1, c2 = GELU_C
    x2 = x * x
    if clamp:
        x2 = torch.clamp(x2, max=GELU_CLAMP)
    p = (c2 * x2 + c1) * x2 + c0
    s = torch.sigmoid(x * p)
    return x2, p, s, (5 * c2 * x2 + 3 * c1) * x2 + c0


def gelu_fit(x, clamp=True):
    """gelu_fwd<false> restated: x * sigmoid(x * (c0 + c1 x^2 + c2 x^4)), x^2 clamped"""
    return x * _fit_parts(x, clamp)[2]


def dgelu_fit(x, clamp=True):
    """gelu_bwd<false> restated: s + x s (1 - s) u'"""
    _, _, s, q = _fit_parts(x, clamp)
    return s + x * (s - s * s) * q


def _gelu_fit32(x, clamp=True):
    """the kernel's operations in fp32 torch (devit_common.h:87-90): exp2 of the product with the -log2(e)-scaled polynomial, a reciprocal"""
    c0, c1, c2 = (torch.tensor(v, dtype=F32) for v in GELU_C)
    l2 = torch.tensor(1.44269504088896341, dtype=F32)
    x2 = x * x
    if clamp:
        x2 = torch.clamp(x2, max=GELU_CLAMP)
    p = ((-c2 * l2) * x2 + (-c1 * l2)) * x2 + (-c0 * l2)
    return x2, 1.0 / (1.0 + torch.exp2(x * p))


def gelu_fit32(x, clamp=True):
    return x * _gelu_fit32(x, clamp)[1]


def dgelu_fit32(x):
    c0, c1, c2 = (torch.tensor(v, dtype=F32) for v in GELU_C)
    x2, s = _gelu_fit32(x)
    q = ((5 * c2) * x2 + 3 * c1) * x2 + c0
    return (x * (s - s * s)) * q + s


def _fit_arith(x):
    """-> (E_s, s, q, Qabs): the fp32 rounding error of s = sigmoid(u) as gelu_fwd / gelu_bwd compute it, for float64 x.
    devit_common.h:87-89 / :100-103: x * x 1, the two fmas 1 each and their three rounded constants (-C LOG2E: 1 on each term) -- 4 on the sum of
    the absolute terms Pabs --, the product x * p 1: |du| <= 5 u |x| Pabs; t = exp2(.) carries du and 2 (v_exp); 1 + t 1; v_rcp 2:
        E_s = s (1 - s) (du + 2 u) + 3 u s"""
    c0, c1, c2 = GELU_C
    x2, _, s, q = _fit_parts(x)
    pabs = abs(c0) + abs(c1) * x2 + abs(c2) * x2 * x2
    du = 5 * U * x.abs() * pabs
    qabs = abs(c0) + 3 * abs(c1) * x2 + 5 * abs(c2) * x2 * x2
    return s * (1 - s) * (du + 2 * U) + 3 * U * s, s, q, qabs


# ============================================================================================ cases
def _case(name, route, M, N, K, kind, **kw):
    c = dict(name=name, route=route, M=M, N=N, K=K, kind=kind, a_km=0, b_km=0, dtype16=0, batch=1, split_k=1, m_valid=0, a_group=0, a_skip=0,
             b_group=0, b_skip=0, aux=False, rowscale=False, alias=False, patch_tokens=0, extra_tokens=0, integer=False, reserve=0, gram=False,
             env=dict(ROUTE_ENV[route]))
    assert set(kw) <= set(c), kw
    c.update(kw)
    return c


def cases():
    """The table.  Shapes are the smallest at which each path exists; PATCH needs m_valid % patch_tokens == 0 (gemm.hip's argument check), so the
    TILE128 PATCH cases take 2 images of 65 tokens (m_valid = 130) and the GEMM4 one 10 images of 196 (m_valid = 1960)."""
    out = []
    add = lambda *a, **k: out.append(_case(*a, **k))                                              # noqa: E731
    # ---- TILE128: M = 256 with m_valid = 130, N = 384; K = 64 is one K-step (the loop body never runs)
    t = dict(m_valid=130)
    for dt, sfx in ((0, "bf16"), (1, "f16")):
        add(f"t128/store_bf16/K192/{sfx}", TILE128, 256, 384, 192, STORE_BF16, dtype16=dt, **t)
        add(f"t128/store_bf16/K64/{sfx}", TILE128, 256, 384, 64, STORE_BF16, dtype16=dt, **t)
        add(f"t128/store_f32/K192/{sfx}", TILE128, 256, 384, 192, STORE_F32, dtype16=dt, **t)
        add(f"t128/gelu/K192/{sfx}", TILE128, 256, 384, 192, GELU, dtype16=dt, aux=True, **t)
        add(f"t128/gelu/K64/{sfx}", TILE128, 256, 384, 64, GELU, dtype16=dt, aux=True, **t)
        add(f"t128/residual/K192/{sfx}", TILE128, 256, 384, 192, RESIDUAL, dtype16=dt, aux=True, rowscale=True, **t)
        add(f"t128/patch_tok2/K192/{sfx}", TILE128, 256, 384, 192, PATCH, dtype16=dt, patch_tokens=65, extra_tokens=2, **t)
        add(f"t128/patch_tok1/K64/{sfx}", TILE128, 256, 384, 64, PATCH, dtype16=dt, patch_tokens=65, extra_tokens=1, **t)
    add("t128/store_f32/K64/bf16", TILE128, 256, 384, 64, STORE_F32, **t)
    add("t128/gelu_noaux/K192/bf16", TILE128, 256, 384, 192, GELU, **t)
    add("t128/residual_alias/K64/bf16", TILE128, 256, 384, 64, RESIDUAL, alias=True, rowscale=True, **t)
    add("t128/residual_plain/K192/bf16", TILE128, 256, 384, 192, RESIDUAL, **t)
    add("t128/store_f32/K192/int", TILE128, 256, 384, 192, STORE_F32, integer=True, **t)
    add("t128/kmB/store_bf16_rowgroup/K192", TILE128, 256, 384, 192, STORE_BF16, b_km=1, b_group=48, b_skip=3, **t)
    add("t128/kmB/store_f32/K64", TILE128, 256, 384, 64, STORE_F32, b_km=1, **t)
    add("t128/kmB/dgelu/K192", TILE128, 256, 384, 192, DGELU, b_km=1, **t)
    add("t128/kmB/dgelu/K64", TILE128, 256, 384, 64, DGELU, b_km=1, **t)
    for sk in (1, 3):
        for aux in (False, True):
            add(f"t128/kmAB/atomic_split{sk}{'_aux' if aux else ''}/K192", TILE128, 256, 384, 192, ATOMIC, a_km=1, b_km=1, split_k=sk, aux=aux, **t)
    add("t128/kmAB/atomic_patch_wgrad/K3136", TILE128, 256, 384, 3136, ATOMIC, a_km=1, b_km=1, split_k=7, aux=True, a_group=196, a_skip=2)
    add("t128/kmAB/atomic_split2/K192/int", TILE128, 256, 384, 192, ATOMIC, a_km=1, b_km=1, split_k=2, aux=True, integer=True)
    add("t128/kmAB/store_f32/K192", TILE128, 256, 384, 192, STORE_F32, a_km=1, b_km=1, **t)
    add("t128/gram_batch3/K64", TILE128, 256, 256, 64, STORE_F32, batch=3, m_valid=198, gram=True)
    # ---- TILE256 (DEVIT_GEMM4=0): M = N = 2048 is 64 tiles, the floor under which gemm.hip falls back to 128x128
    w = dict(m_valid=1922)
    for dt, sfx in ((0, "bf16"), (1, "f16")):
        add(f"t256/store_bf16/K384/{sfx}", TILE256, 2048, 2048, 384, STORE_BF16, dtype16=dt, **w)
        add(f"t256/store_f32/K384/{sfx}", TILE256, 2048, 2048, 384, STORE_F32, dtype16=dt, **w)
        add(f"t256/gelu/K64/{sfx}", TILE256, 2048, 2048, 64, GELU, dtype16=dt, aux=True, **w)
        add(f"t256/gelu/K192/{sfx}", TILE256, 2048, 2048, 192, GELU, dtype16=dt, aux=True, **w)
        add(f"t256/residual/K1536/{sfx}", TILE256, 2048, 2048, 1536, RESIDUAL, dtype16=dt, aux=True, rowscale=True, **w)
        add(f"t256/patch/K768/{sfx}", TILE256, 2304, 2048, 768, PATCH, dtype16=dt, patch_tokens=196, extra_tokens=2, m_valid=2156)
    add("t256/store_f32/K384/int", TILE256, 2048, 2048, 384, STORE_F32, integer=True, **w)
    add("t256/kmB/store_bf16/K384", TILE256, 2048, 2048, 384, STORE_BF16, b_km=1, **w)
    add("t256/kmB/store_f32/K384", TILE256, 2048, 2048, 384, STORE_F32, b_km=1, **w)
    add("t256/kmB/dgelu/K64", TILE256, 2048, 2048, 64, DGELU, b_km=1, **w)
    r = dict(m_valid=3200)
    add("t256/ragged/store_bf16/K384", TILE256, 3328, 1152, 384, STORE_BF16, **r)
    add("t256/ragged/gelu/K384", TILE256, 3328, 1152, 384, GELU, aux=True, **r)
    add("t256/ragged/kmB_dgelu/K384", TILE256, 3328, 1152, 384, DGELU, b_km=1, **r)
    add("t256/batch64/store_f32/K384", TILE256, 256, 256, 384, STORE_F32, batch=64, m_valid=198)
    # ---- GEMM4 (DEVIT_GEMM4=1): K = 192 is the shortest loop it accepts
    add("g4/gelu/K192", GEMM4, 2048, 2048, 192, GELU, aux=True, **w)
    add("g4/store_bf16/K384", GEMM4, 2048, 2048, 384, STORE_BF16, **w)
    add("g4/store_f32/K384", GEMM4, 2048, 2048, 384, STORE_F32, **w)
    add("g4/store_f32/K384/int", GEMM4, 2048, 2048, 384, STORE_F32, integer=True, **w)
    add("g4/residual/K768", GEMM4, 2048, 2048, 768, RESIDUAL, aux=True, rowscale=True, **w)
    add("g4/patch/K768", GEMM4, 2048, 2048, 768, PATCH, patch_tokens=196, extra_tokens=2, m_valid=1960)
    # ---- FULL_ROW (DEVIT_GEMMFR=1): k-major B, N = 384
    f = dict(b_km=1, m_valid=300)
    add("fr/store_bf16/K192", FULL_ROW, 512, 384, 192, STORE_BF16, **f)
    add("fr/residual/K256", FULL_ROW, 512, 384, 256, RESIDUAL, rowscale=True, aux=True, **f)
    add("fr/residual_alias/K192", FULL_ROW, 512, 384, 192, RESIDUAL, rowscale=True, alias=True, **f)
    add("fr/residual/K256/int", FULL_ROW, 512, 384, 256, RESIDUAL, rowscale=True, integer=True, **f)
    # ---- more than one tile per workgroup: with 128 CUs reserved a 256-CU device runs 128 (256x256, full-row) or 256 (128x128) workgroups
    add("multi/t256/gelu/K192", TILE256, 4352, 2048, 192, GELU, reserve=128, aux=True, m_valid=4300)
    add("multi/g4/residual/K768", GEMM4, 4352, 2048, 768, RESIDUAL, reserve=128, rowscale=True, aux=True, m_valid=4300)
    add("multi/t128/gelu/K64", TILE128, 2176, 2048, 64, GELU, reserve=128, aux=True, m_valid=2100)
    add("multi/fr/store_bf16/K192", FULL_ROW, 33024, 384, 192, STORE_BF16, reserve=128, b_km=1, m_valid=33000)
    names = [c["name"] for c in out]
    assert len(set(names)) == len(names)
    return out


def set_route_env(monkeypatch, c):
    """put the process on the case's route: both per-call switches cleared, then the case's own set.  DEVIT_GEMM_FORCE is read once per process and
    overrides the selection rule under test: with it set the test skips with that reason."""
    import pytest
    if os.environ.get("DEVIT_GEMM_FORCE"):
        pytest.skip("DEVIT_GEMM_FORCE is set in the environment: it is read once per process and overrides the selection rule under test")
    for k in ROUTE_SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in c["env"].items():
        monkeypatch.setenv(k, v)


def tiles_of(c):
    """(tile rows, tile columns, workgroups per CU) of the case's route.  A restatement of gemm_launch (gemm.hip: `bm`, `bn` and `occ`), used only
    for the premise of the `reserve` cases and the count of row-sum atomics; the route itself is always asked of devit_gemm_route."""
    return {TILE128: (128, 128, 2), TILE256: (256, 256, 1), GEMM4: (256, 256, 1), FULL_ROW: (256, 384, 1)}[c["route"]]


def tile_count(c):
    bm, bn, _ = tiles_of(c)
    return (c["M"] // bm) * ((c["N"] + bn - 1) // bn) * c["split_k"] * c["batch"]


def instantiation(c):
    """(route, layout variant = 2 (A k-major) + (B k-major), kind, dtype16): the kernel instantiation the case runs"""
    return (c["route"], 2 * c["a_km"] + c["b_km"], c["kind"], c["dtype16"])


def case_named(name):
    return next(c for c in cases() if c["name"] == name)


# ============================================================================================ inputs
def t16(c):
    return F16 if c["dtype16"] else BF16


def phys_row(r, group, skip, mutate=None):
    """devit_operand: the physical row of reduction row r is r + skip * (r / group + 1) (gemm_device.h:33-35)"""
    if group <= 0:
        return r
    return r + skip * (torch.div(r, group, rounding_mode="floor") + (0 if mutate == "row_skip_without_plus_one" else 1))


def _operand(rows, K, km, group, skip, vals, dt, nan_rows=None):
    """a [rows][K] logical matrix `vals` laid out as devit_operand describes it, ld = width + PAD; everything the description does not name is NaN
    -> (flat buffer, descriptor)"""
    k = torch.arange(K)
    if km:
        pk = phys_row(k, group, skip)
        nphys = int(pk[-1]) + 1
        ld = rows + PAD
        buf = torch.full((nphys, ld), NAN, dtype=dt)
        buf[pk, :rows] = vals.t().to(dt)
    else:
        ld = K + PAD
        buf = torch.full((rows, ld), NAN, dtype=dt)
        buf[:, :K] = vals.to(dt)
    return buf.reshape(-1), dict(off=0, ld=ld, km=km, group=group, skip=skip, bs=0)


def _row_powers(g, rows):
    """2^-6 .. 2^6 by row (exact in both 16-bit types): a matrix-max norm sees only the largest rows"""
    return 2.0 ** (torch.randperm(rows, generator=g) % 13 - 6).to(F32)


def inputs(c):
    """Seeded CPU tensors of a case: {bufs: name -> flat tensor, A / B: operand descriptors, geometry of the outputs}.  See the module docstring for
    what holds NaN and what holds the sentinel."""
    g = gen("gemm", c["name"])
    M, N, K, kind, batch, dt = c["M"], c["N"], c["K"], c["kind"], c["batch"], t16(c)
    m_lim = c["m_valid"] or M
    ldc = N + PAD
    bufs = {}
    if c["gram"]:
        # relation_loss: the q and k features of `batch` images of 198 tokens in ONE [rows][2 K] buffer, windows of 256 rows 198 apart (a window reads
        # the next image's rows -- finite data -- and its rows >= 198 are not stored); both operands are views of that buffer
        rows, ld = 198 * batch + 128, 2 * K + PAD
        buf = torch.full((rows, ld), NAN, dtype=dt)
        buf[:, :2 * K] = (torch.randn(rows, 2 * K, generator=g) * _row_powers(g, rows)[:, None] / 8).to(dt)
        bufs["ab"] = buf.reshape(-1)
        A = dict(buf="ab", off=0, ld=ld, km=0, group=0, skip=0, bs=198 * ld)
        B = dict(buf="ab", off=K, ld=ld, km=0, group=0, skip=0, bs=198 * ld)
    else:
        if c["integer"]:
            a = torch.randint(-4, 5, (M, K), generator=g).to(F32)
            b = torch.randint(-4, 5, (N, K), generator=g).to(F32)
        else:
            a = torch.randn(M, K, generator=g) * _row_powers(g, M)[:, None]
            b = torch.randn(N, K, generator=g) / math.sqrt(K)
        if not c["a_km"] and m_lim < M and batch == 1:     # rows of a row-major A at or above m_valid: read, never stored -- finite junk and one inf
            a[m_lim:] = torch.randn(M - m_lim, K, generator=g) * 100
            a[M - 1, K // 2] = math.inf
        if batch > 1:                                       # batched operands: `batch` matrices behind one another, a gap of PAD rows between them
            a = torch.randn(batch, M, K, generator=g) * _row_powers(g, M)[None, :, None]
            b = torch.randn(batch, N, K, generator=g) / math.sqrt(K)
            fa, A = zip(*[_operand(M, K, 0, 0, 0, a[z], dt) for z in range(batch)])
            fb, B = zip(*[_operand(N, K, 0, 0, 0, b[z], dt) for z in range(batch)])
            gap = torch.full((PAD * 8,), NAN, dtype=dt)
            bufs["a"] = torch.cat([torch.cat([x, gap]) for x in fa])
            bufs["b"] = torch.cat([torch.cat([x, gap]) for x in fb])
            A, B = dict(A[0], bs=fa[0].numel() + gap.numel()), dict(B[0], bs=fb[0].numel() + gap.numel())
        else:
            bufs["a"], A = _operand(M, K, c["a_km"], c["a_group"], c["a_skip"], a, dt)
            bufs["b"], B = _operand(N, K, c["b_km"], c["b_group"], c["b_skip"], b, dt)
        A["buf"], B["buf"] = "a", "b"

    def colvec(v):
        return torch.cat([v.to(F32), torch.full((PAD,), NAN)])

    ints = c["integer"]
    if kind not in (DGELU, ATOMIC):
        mag = 10 ** (torch.rand(N, generator=g) * (math.log10(30) + 3) - 3)                  # 1e-3 .. 30 by column
        sign = torch.where(torch.rand(N, generator=g) < 0.5, -1.0, 1.0)
        bufs["bias"] = colvec(torch.randint(-9, 10, (N,), generator=g).to(F32) if ints else mag * sign)
    if kind in (GELU, DGELU):
        bufs["colscale"] = colvec(torch.tensor(COLSCALES)[torch.randint(0, 5, (N,), generator=g)])
    # ---- the output side: [out_rows][ldc] per batch, pad columns and a guard behind the end hold SENT
    T, tok = c["patch_tokens"], c["extra_tokens"]
    out_rows = (m_lim // T) * (T + tok) if kind == PATCH else M
    out_bs = out_rows * ldc + 8 * PAD if batch > 1 else 0
    n_flat = (out_rows * ldc + 8 * PAD) * batch + GUARD
    geo = dict(ldc=ldc, out_rows=out_rows, out_bs=out_bs, n_flat=n_flat, m_lim=m_lim)
    odt = dt if kind in OUT16 else F32
    out0 = torch.full((n_flat,), SENT, dtype=odt)
    live = live_index(c, geo)
    if kind == ATOMIC:                                    # the accumulator is preloaded
        out0[live.reshape(-1)] = (torch.randint(-50, 51, live.shape, generator=g) if ints else torch.randn(live.shape, generator=g) * 3).to(F32).reshape(-1)
        if c["aux"]:
            aux0 = torch.full((M + GUARD,), SENT, dtype=F32)
            aux0[:m_lim] = torch.randint(-50, 51, (m_lim,), generator=g).to(F32) if ints else torch.randn(m_lim, generator=g) * 3
            bufs["aux0"] = aux0
    elif c["aux"]:
        bufs["aux0"] = torch.full((n_flat,), SENT, dtype=dt)
    if kind == RESIDUAL:
        resv = (torch.randint(-50, 51, live.shape, generator=g).to(F32) if ints
                else torch.randn(live.shape, generator=g) * 2.0 ** (torch.arange(live.shape[1]) % 5)[None, :, None])
        if c["alias"]:
            out0[live.reshape(-1)] = resv.reshape(-1)     # res IS out: its rows >= m_valid and pad columns are the sentinel that must come back
        else:
            res = torch.full((n_flat,), NAN, dtype=F32)
            res[live.reshape(-1)] = resv.reshape(-1)
            bufs["res"] = res
        if c["rowscale"]:
            rps = 198 if M >= 1024 else 33
            n = (m_lim + rps - 1) // rps
            rs = torch.tensor((0.0, 1.0, 2.0) if ints else ROWSCALES)[torch.randint(0, 3 if ints else 4, (n,), generator=g)]
            bufs["rowscale"] = torch.cat([rs.to(F32), torch.full((PAD,), NAN)])
            geo["rows_per_scale"] = rps
    if kind == PATCH:
        pos = torch.full((tok + T, ldc), NAN)             # rows 0 .. tok-1 (cls / dist, written by devit_embed_tokens) are not this kernel's to read
        pos[tok:, :N] = torch.randn(T, N, generator=g) * 0.05
        bufs["pos"] = pos.reshape(-1)
    if kind == DGELU:
        pre = torch.full((n_flat,), NAN, dtype=dt)        # saved pre-activation, out's geometry: spread over [-12, 12]
        pre[live.reshape(-1)] = ((torch.rand(live.shape, generator=g) * 24 - 12).to(dt)).reshape(-1)
        bufs["aux_in"] = pre
    bufs["out0"] = out0
    return dict(bufs=bufs, A=A, B=B, geo=geo)


def live_index(c, geo):
    """[batch][m_lim][N] flat indices of the output elements the call must write (PATCH: the token-row remap, gemm_device.h:258-263)"""
    m = torch.arange(geo["m_lim"])
    if c["kind"] == PATCH:
        T, tok = c["patch_tokens"], c["extra_tokens"]
        m = torch.div(m, T, rounding_mode="floor") * (T + tok) + tok + m % T
    z = torch.arange(c["batch"])
    return z[:, None, None] * geo["out_bs"] + m[None, :, None] * geo["ldc"] + torch.arange(c["N"])[None, None, :]


def to_device(inp, dev):
    return dict(inp, bufs={k: v.to(dev) for k, v in inp["bufs"].items()})


def logical(inp, d, rows, K, batch, mutate=None):
    """[batch][rows][K]: the matrix the operand description `d` names, gathered from its flat buffer"""
    buf = inp["bufs"][d["buf"]]
    dev = buf.device
    r, k, z = torch.arange(rows, device=dev), torch.arange(K, device=dev), torch.arange(batch, device=dev)
    if d["km"]:
        idx = phys_row(k, d["group"], d["skip"], mutate)[None, :] * d["ld"] + r[:, None]
    else:
        idx = r[:, None] * d["ld"] + k[None, :]
    return buf[d["off"] + z[:, None, None] * d["bs"] + idx[None]]


def call_args(c, inp, at):
    """(args, kwargs) of ops.gemm / ops.gemm_route for the case.  at(name, off) -> what stands for buffer `name` from element `off` on: a tensor view
    for a launch, any 16-byte aligned address for a route query ('out' / 'aux' name the buffers the call writes)."""
    geo, A, B, bufs = inp["geo"], inp["A"], inp["B"], inp["bufs"]
    opt = lambda n: at(n, 0) if n in bufs else None                                            # noqa: E731
    kw = dict(kind=c["kind"], out=at("out", 0), ldc=geo["ldc"], bias=opt("bias"), colscale=opt("colscale"), aux=at("aux", 0) if "aux0" in bufs else None,
              aux_in=opt("aux_in"), res=at("out", 0) if c["alias"] else opt("res"), rowscale=opt("rowscale"), rows_per_scale=geo.get("rows_per_scale", 0),
              pos=opt("pos"), patch_tokens=c["patch_tokens"], extra_tokens=c["extra_tokens"], batch=c["batch"], a_bs=A["bs"], b_bs=B["bs"],
              out_bs=geo["out_bs"], m_valid=c["m_valid"], split_k=c["split_k"], a_group=A["group"], a_skip=A["skip"], b_group=B["group"],
              b_skip=B["skip"], dtype16=c["dtype16"])
    return (at(A["buf"], A["off"]), A["ld"], A["km"], at(B["buf"], B["off"]), B["ld"], B["km"], c["M"], c["N"], c["K"]), kw


def fake_address(name, off):
    """an aligned non-null address per buffer for a route query (devit_gemm_route dereferences no data pointer)"""
    return 0x100000 * (1 + sum(ord(ch) for ch in name) % 97) + 4 * off


# ============================================================================================ reference and bounds
def _live(inp, c, name):
    return inp["bufs"][name][live_index(c, inp["geo"]).to(inp["bufs"][name].device)]


def statement(kind, a, b, *, bias=None, colscale=None, rowscale=None, res=None, aux_in=None, pos=None, f16=False, aux=False, out0=None,
              aux0=None, split_k=1, tiles_n=1):
    """One launch of devit_gemm_bf16 on LOGICAL float64 matrices, exactly as include/devit_hip.h words each kind -> (ref, bnd): dicts over 'out' and,
    where the launch writes one, 'aux'.  a [..][m][K] and b [..][N][K] hold the 16-bit operands exactly; bias / colscale [N]; rowscale broadcastable
    to the output with the scale of every row already looked up (None: 1); res / aux_in / pos in the output's shape; ATOMIC: out0 / aux0 what the
    accumulators held, split_k the slices, tiles_n the n-tiles that each add a share of a row sum.  reference() gathers these from a case's
    physical buffers; tests/_block_model.py feeds it the buffers an encoder block left behind."""
    K = a.shape[-1]
    acc = a @ b.transpose(-1, -2)
    absacc = a.abs() @ b.abs().transpose(-1, -2)
    cs = colscale
    ref, bnd = {}, {}
    if kind == ATOMIC:
        # out += acc; aux[m] += sum_k A[m][k].  s: one atomic per slice (gemm_tile.h:385), the preloaded value is a term of the sum
        ref["out"] = out0 + acc
        bnd["out"] = E32 * (K + split_k) * (absacc + out0.abs())
        if aux:
            # sum8_bf16 (gemm_tile.h:9-16): K additions; the folds 2 (:397-398); one atomic per (slice, n-tile) that took a K-step (:305,400)
            a0 = a[0] if a.dim() == 3 else a
            ref["aux"] = aux0 + a0.sum(1)
            bnd["aux"] = E32 * (K + 2 + split_k * tiles_n) * (a0.abs().sum(1) + aux0.abs())
        return ref, bnd
    e_acc = E32 * K * absacc                               # s = 0: the accumulators start at zero and one workgroup owns the whole K
    if kind == DGELU:
        # out = acc * colscale * gelu'(aux_in) (gemm_device.h:360,367): acc + 0 is exact; acc * cs 1; gelu_bwd's arithmetic E_g; the product 1.
        # gelu_bwd (devit_common.h:100-104): q 3 on Qabs; w = fma(-s, s, s) carries |1 - 2 s| E_s and 1; x * w 1; fma(x w, q, s) 1 on the result
        z = aux_in
        e_s, s, q, qabs = _fit_arith(z)
        w = s * (1 - s)
        e_w = (1 - 2 * s).abs() * e_s + U * w
        g = dgelu_exact(z)
        e_g = DGELU_FIT_ERR + q.abs() * z.abs() * (e_w + U * w) + (z * w).abs() * 3 * U * qabs + e_s + U * g.abs()
        ref["out"] = acc * cs * g
        bnd["out"] = stored16(cs.abs() * g.abs() * e_acc + (acc * cs).abs() * e_g + 2 * U * ref["out"].abs(), ref["out"], f16)
        return ref, bnd
    pre = acc + bias if bias is not None else acc
    e_pre = e_acc + U * pre.abs()                          # gemm_device.h:300 / :360: acc + bias, one rounding
    if kind == STORE_F32:
        ref["out"], bnd["out"] = pre, e_pre
    elif kind == STORE_BF16:
        ref["out"], bnd["out"] = pre, stored16(e_pre, pre, f16)
    elif kind == GELU:
        # out = gelu(acc + bias) * colscale on the fp32 x (gemm_device.h:364); aux = the same x rounded to 16 bits (:362).
        # gelu_fwd (devit_common.h:87-90): s as _fit_arith; x * s 1; times cs 1 (gemm_device.h:364)
        e_s, s, _, _ = _fit_arith(pre)
        ref["out"] = gelu_exact(pre) * cs
        e = cs.abs() * (dgelu_exact(pre).abs() * e_pre + GELU_FIT_ERR + pre.abs() * e_s + U * (pre * s).abs()) + U * ref["out"].abs()
        bnd["out"] = stored16(e, ref["out"], f16)
        if aux:
            ref["aux"], bnd["aux"] = pre, stored16(e_pre, pre, f16)
    elif kind == RESIDUAL:
        # out = res + rowscale[m / rows_per_scale] * (acc + bias) (gemm_device.h:316): the product 1, the sum 1; aux = cvt(acc + bias) (:305)
        rs = rowscale if rowscale is not None else torch.ones((), dtype=F64, device=res.device)
        ref["out"] = res + rs * pre
        bnd["out"] = rs.abs() * e_pre + U * (rs * pre).abs() + U * ref["out"].abs()
        if aux:
            ref["aux"], bnd["aux"] = pre, stored16(e_pre, pre, f16)
    elif kind == PATCH:
        # row m = (b, t): out[b (T + tok) + tok + t] = acc + bias + pos[tok + t] (gemm_device.h:286,315): one more sum
        ref["out"] = pre + pos
        bnd["out"] = e_pre + U * ref["out"].abs()
    return ref, bnd


def reference(c, inp, with_bounds=True):
    """-> (ref, bnd): float64 [batch][m_lim][N] per output name ('out', 'aux'; ATOMIC aux: [m_lim]): statement() on the logical matrices that the
    case's operand descriptions name."""
    geo, kind, K, N = inp["geo"], c["kind"], c["K"], c["N"]
    m_lim = geo["m_lim"]
    a = logical(inp, inp["A"], m_lim, K, c["batch"]).to(F64)
    b = logical(inp, inp["B"], N, K, c["batch"]).to(F64)
    bufs = inp["bufs"]
    vec = lambda n: bufs[n][:N].to(F64) if n in bufs else None                                 # noqa: E731
    kw = dict(bias=vec("bias"), colscale=vec("colscale"), f16=bool(c["dtype16"]), aux=bool(c["aux"]))
    if kind == ATOMIC:
        kw.update(out0=_live(inp, c, "out0").to(F64), split_k=c["split_k"], tiles_n=(N + tiles_of(c)[1] - 1) // tiles_of(c)[1])
        if c["aux"]:
            kw["aux0"] = bufs["aux0"][:m_lim].to(F64)
    elif kind == DGELU:
        kw["aux_in"] = _live(inp, c, "aux_in").to(F64)
    elif kind == RESIDUAL:
        kw["res"] = _live(inp, c, "out0" if c["alias"] else "res").to(F64)
        if c["rowscale"]:
            m = torch.arange(m_lim, device=kw["res"].device)
            kw["rowscale"] = bufs["rowscale"].to(F64)[torch.div(m, geo["rows_per_scale"], rounding_mode="floor")][None, :, None]
    elif kind == PATCH:
        T, tok = c["patch_tokens"], c["extra_tokens"]
        t = torch.arange(m_lim, device=a.device) % T
        kw["pos"] = bufs["pos"].view(tok + T, geo["ldc"])[tok + t, :N].to(F64)[None]
    return statement(kind, a, b, **kw)


# ============================================================================================ emulation
def emulate(c, inp, mutate=None):
    """-> {name: flat buffer as the call leaves it}: fp32 torch, K in blocks of 64 (every split-K slice summed apart and added in turn), the
    kernel's fitted GELU, 16-bit stores by one rounding.  `mutate`: one of MUTATIONS."""
    assert mutate is None or mutate in MUTATIONS
    geo, kind, K, N, M = inp["geo"], c["kind"], c["K"], c["N"], c["M"]
    m_lim, dt = geo["m_lim"], t16(c)
    bufs = inp["bufs"]
    rows = min(M, m_lim + 1) if mutate == "m_valid_plus_one" else m_lim        # (one row too many stored)
    a = logical(inp, inp["A"], rows, K, c["batch"], mutate).to(F32)
    b = logical(inp, inp["B"], N, K, c["batch"], mutate).to(F32)
    if mutate == "last_product_dropped":
        a = a.clone()
        a[:, :, K - 1] = 0
    nk = K // 64
    parts = []
    for z in range(c["split_k"]):
        k0, k1 = z * nk // c["split_k"], (z + 1) * nk // c["split_k"]
        p = torch.zeros(c["batch"], rows, N)
        for t in range(k0, k1):
            p = p + a[:, :, 64 * t:64 * t + 64] @ b[:, :, 64 * t:64 * t + 64].transpose(1, 2)
        parts.append(p)
    if mutate == "split_slice_twice":
        parts.append(parts[-1])
    geo_m = dict(geo, m_lim=rows)
    idx = live_index(c, geo_m).reshape(-1)
    got = {"out": bufs["out0"].clone()}
    if "aux0" in bufs:
        got["aux"] = bufs["aux0"].clone()

    def put(name, v):
        got[name][idx] = v.to(got[name].dtype).reshape(-1)

    def cvt(v):
        return v.to(BF16).to(dt) if mutate == "f16_store_through_bf16" else v.to(dt)

    if kind == ATOMIC:
        o = got["out"][idx].view(c["batch"], rows, N)
        for p in parts:
            o = o + p
        put("out", o)
        if c["aux"]:
            s = got["aux"][:rows].clone()
            for z in range(c["split_k"]):
                k0, k1 = z * nk // c["split_k"], (z + 1) * nk // c["split_k"]
                s = s + a[0][:, 64 * k0:64 * k1].sum(1)
            got["aux"][:rows] = s
        return got
    acc = parts[0]
    vec = lambda n: bufs[n][:N].to(F32) if n in bufs else None                                 # noqa: E731
    bias, cs = vec("bias"), vec("colscale")
    if bias is not None and mutate == "bias_from_left_at_tile_edge":
        n = torch.arange(N)
        bias = bias[torch.where((n % 128 == 0) & (n > 0), n - 1, n)]
    if kind == DGELU:
        z = bufs["aux_in"][live_index(c, geo_m)].to(F32)
        put("out", cvt(acc * cs * dgelu_fit32(z)))
        return got
    pre = acc + bias if bias is not None else acc
    if kind == STORE_F32:
        put("out", pre)
    elif kind == STORE_BF16:
        put("out", cvt(pre))
    elif kind == GELU:
        put("out", cvt(gelu_fit32(pre, clamp=mutate != "gelu_without_clamp") * cs))
        if c["aux"]:
            put("aux", cvt(pre * cs if mutate == "colscale_on_saved_preactivation" else pre))
    elif kind == RESIDUAL:
        res = bufs["out0" if c["alias"] else "res"][live_index(c, geo_m)].to(F32)
        if c["rowscale"]:
            m = torch.arange(rows)
            if mutate == "rowscale_tile_local":
                m = m % tiles_of(c)[0]
            rs = bufs["rowscale"][torch.div(m, geo["rows_per_scale"], rounding_mode="floor")][None, :, None]
        else:
            rs = torch.ones(())
        put("out", res + rs * pre)
        if c["aux"]:
            put("aux", cvt(pre))
    elif kind == PATCH:
        T, tok = c["patch_tokens"], c["extra_tokens"]
        t = torch.arange(rows) % T
        pos = bufs["pos"].view(tok + T, geo["ldc"])[(0 if mutate == "patch_without_tok" else tok) + t, :N][None]
        put("out", pre + pos)
    return got


# ============================================================================================ verdict
def verdict(c, inp, got, ref_bnd=None):
    """-> ({output name: worst |err| / bound over EVERY live element}, untouched): untouched is True when every element of every output buffer that
    the call must not write (rows >= m_valid, pad columns, the gaps between batches, the token rows of a PATCH output, the guard) is bit-unchanged.
    An exact-integer case reports 0 where torch.equal holds against the float64 statement and inf where it does not."""
    ref, bnd = ref_bnd or reference(c, inp)
    geo, bufs = inp["geo"], inp["bufs"]
    idx = live_index(c, geo).to(got["out"].device)
    rt, untouched = {}, True
    for name in ref:
        g, init = got[name], bufs["aux0" if name == "aux" else "out0"].to(got[name].device)
        if c["kind"] == ATOMIC and name == "aux":
            live, mask = g[:geo["m_lim"]], torch.zeros(g.numel(), dtype=torch.bool, device=g.device)
            mask[:geo["m_lim"]] = True
        else:
            live, mask = g[idx], torch.zeros(g.numel(), dtype=torch.bool, device=g.device)
            mask[idx.reshape(-1)] = True
        untouched = untouched and torch.equal(g[~mask].view(torch.int16 if g.element_size() == 2 else torch.int32),
                                              init[~mask].view(torch.int16 if g.element_size() == 2 else torch.int32))
        if c["integer"]:
            rt[name] = 0.0 if torch.equal(live.to(F64), ref[name]) else math.inf
        else:
            rt[name] = ratio(live, ref[name], bnd[name])
    return rt, untouched


# ============================================================================================ devit_wgrad_grouped (wgradfr.hip)
W_B = 384          # the operand that is exactly 384 columns wide


def _wjob(name, a_cols, transposed=0, lda_extra=PAD, colsum=True):
    return dict(name=name, a_cols=a_cols, transposed=transposed, lda_extra=lda_extra, colsum=colsum)


def wgrad_cases():
    """(name, K reduction rows, split_k as passed (0: the entry point's cost model chooses), jobs).  a_cols 128 is only the half tile."""
    jobs = [_wjob("half", 128), _wjob("one_and_half", 384, colsum=False), _wjob("wide_t", 1152, transposed=1),
            _wjob("wide_lda", 384, lda_extra=136), _wjob("half_t", 128, transposed=1, colsum=False)]
    return [("K192_split1", 192, 1, jobs), ("K576_split3", 576, 3, jobs), ("K576_split0", 576, 0, jobs),
            ("K192_48_jobs", 192, 1, [_wjob(f"j{i}", 128, colsum=i % 2 == 0) for i in range(48)]),
            ("K192_int", 192, 1, [dict(_wjob("int", 384), integer=True), dict(_wjob("int_t", 128, transposed=1), integer=True)])]


def wgrad_inputs(name, K, jobs):
    """per job: a [K][lda] and b [K][ldb] 16-bit with NaN in the columns past a_cols / 384, out0 / colsum0 preloaded accumulators with SENT in their
    pad columns and guards.  (Rows >= K do not exist: the buffers end there.)"""
    out = []
    for j in jobs:
        g = gen("wgrad", name, j["name"])
        ac, lda, ldb = j["a_cols"], j["a_cols"] + j["lda_extra"], W_B + PAD
        ints = j.get("integer", False)
        a = torch.full((K, lda), NAN, dtype=BF16)
        b = torch.full((K, ldb), NAN, dtype=BF16)
        if ints:
            a[:, :ac] = torch.randint(-4, 5, (K, ac), generator=g).to(BF16)
            b[:, :W_B] = torch.randint(-4, 5, (K, W_B), generator=g).to(BF16)
        else:
            a[:, :ac] = (torch.randn(K, ac, generator=g) * _row_powers(g, ac)[None, :]).to(BF16)
            b[:, :W_B] = (torch.randn(K, W_B, generator=g) / math.sqrt(K)).to(BF16)
        orows, ocols = (W_B, ac) if j["transposed"] else (ac, W_B)
        ldc = ocols + PAD
        out0 = torch.full((orows * ldc + GUARD,), SENT, dtype=F32)
        v = out0[:orows * ldc].view(orows, ldc)
        v[:, :ocols] = torch.randint(-50, 51, (orows, ocols), generator=g).to(F32) if ints else torch.randn(orows, ocols, generator=g) * 3
        d = dict(job=j, a=a, b=b, lda=lda, ldb=ldb, ldc=ldc, orows=orows, ocols=ocols, out0=out0)
        if j["colsum"]:
            c0 = torch.full((ac + GUARD,), SENT, dtype=F32)
            c0[:ac] = torch.randint(-50, 51, (ac,), generator=g).to(F32) if ints else torch.randn(ac, generator=g) * 3
            d["colsum0"] = c0
        out.append(d)
    return out


def wgrad_max_split(K):
    """the most slices split_k == 0 can choose (wgradfr.hip:267: sk <= 64 and nk_total / sk >= 3)"""
    return max(1, min(64, K // 64 // 3))


def wgrad_reference(d, K, split):
    """out[i][j] += sum_k a[k][i] b[k][j] (transposed: out[j][i]); a_colsum[i] += sum_k a[k][i].  s = `split` atomics (wgradfr.hip:173-175,182) and the
    preloaded value; the column sums: K additions (v_dot2c against ones), 2 folds (:217-218), one atomic per slice (:221)."""
    a, b = d["a"][:, :d["job"]["a_cols"]].to(F64), d["b"][:, :W_B].to(F64)
    acc, absacc = a.t() @ b, a.abs().t() @ b.abs()
    if d["job"]["transposed"]:
        acc, absacc = acc.t(), absacc.t()
    out0 = d["out0"][:d["orows"] * d["ldc"]].view(d["orows"], d["ldc"])[:, :d["ocols"]].to(F64)
    ref, bnd = {"out": out0 + acc}, {"out": E32 * (K + split) * (absacc + out0.abs())}
    if "colsum0" in d:
        c0 = d["colsum0"][:d["job"]["a_cols"]].to(F64)
        ref["colsum"], bnd["colsum"] = c0 + a.sum(0), E32 * (K + 2 + split) * (a.abs().sum(0) + c0.abs())
    return ref, bnd


def wgrad_emulate(d, K, split, mutate=None):
    a, b = d["a"][:, :d["job"]["a_cols"]].to(F32), d["b"][:, :W_B].to(F32)
    got = {"out": d["out0"].clone()}
    o = got["out"][:d["orows"] * d["ldc"]].view(d["orows"], d["ldc"])[:, :d["ocols"]]
    nk = K // 64
    for z in range(split):
        k0, k1 = 64 * (z * nk // split), 64 * ((z + 1) * nk // split)
        p = a[k0:k1].t() @ b[k0:k1]
        o += p.t() if d["job"]["transposed"] else p
    if "colsum0" in d:
        got["colsum"] = d["colsum0"].clone()
        # a_colsum is over a's columns whichever way `out` lies (wgradfr.hip:211-222); the planted bug takes the 384-wide operand instead -- the one a
        # transposed job's output ROWS follow -- wrapped where a_cols exceeds 384
        ac = d["job"]["a_cols"]
        sums = b.sum(0)[torch.arange(ac) % W_B] if mutate == "colsum_of_wrong_operand" else a.sum(0)
        got["colsum"][:ac] += sums
    return got


def wgrad_verdict(d, got, ref_bnd):
    ref, bnd = ref_bnd
    ints = d["job"].get("integer", False)
    o = got["out"][:d["orows"] * d["ldc"]].view(d["orows"], d["ldc"])
    init = d["out0"].to(o.device)
    untouched = torch.equal(o[:, d["ocols"]:], init[:d["orows"] * d["ldc"]].view(d["orows"], d["ldc"])[:, d["ocols"]:]) and \
        torch.equal(got["out"][d["orows"] * d["ldc"]:], init[d["orows"] * d["ldc"]:])
    live = {"out": o[:, :d["ocols"]]}
    if "colsum" in ref:
        ac = d["job"]["a_cols"]
        untouched = untouched and torch.equal(got["colsum"][ac:], d["colsum0"].to(o.device)[ac:])
        live["colsum"] = got["colsum"][:ac]
    rt = {k: (0.0 if torch.equal(live[k].to(F64), ref[k]) else math.inf) if ints else ratio(live[k], ref[k], bnd[k]) for k in ref}
    return rt, untouched
