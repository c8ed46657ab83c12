"""The kernels behind the C ABI that are neither GEMM, attention, dropout, HSIC nor the optimizer (tests/test_gpu_optim.py) -- LayerNorm, the
elementwise helpers, the losses, the index copies and the exact-fp32 companions -- on a real MI355X against the float64 statements of tests/_tail_model.py, on the inputs
tests/test_tail_model.py holds the model itself to.  Three kinds of assertion, the strongest that applies:
    bit-exact   (torch.equal) where the op is a copy or one correctly rounded operation, against the same operation in torch fp32;
    exact ints  small-integer inputs whose every partial sum is representable, against int64 / float64 arithmetic;
    bounded     chk(worst |err| / bound, 1.0, name="tail/<kernel>/<case>/<output>") with the elementwise bound derived in _tail_model.
Every output buffer has guard elements behind it and in its ld - N pad columns, holding a sentinel that must come back; inputs a kernel must
not consume hold NaN; outputs a call must overwrite start as NaN.  Every refusal below is the entry point's argument check: nothing is launched."""
import ctypes as C
import math

import pytest
import torch

import _tail_model as T
from _tail_model import BF16, F16, F32, F64, ratio, stored16
from conftest import chk

pytestmark = pytest.mark.gpu

SENT = -123.0          # exact in bf16, f16 and fp32
GUARD = 64
NAN = math.nan


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from devit_amd import _lib
    _lib.require_device(torch.zeros(1, device="cuda"))
    return torch.device("cuda")


def _L():
    from devit_amd import _lib
    return _lib


def call(name, *args):
    L = _L()
    return L.call(name, *[L.ptr(a) if isinstance(a, torch.Tensor) else a for a in args], L.stream_ptr())


def refused(name, *args):
    with pytest.raises(_L().DevitError):
        call(name, *args)


class Out:
    """[rows][ld] with `cols` live columns inside a flat allocation: pad columns and GUARD elements behind the end hold SENT; the live part starts as
    `init` (a tensor, or NaN: the call must overwrite it)"""

    def __init__(self, dev, rows, cols, dtype=F32, ld=None, init=NAN):
        self.rows, self.cols, self.ld = rows, cols, cols if ld is None else ld
        self.flat = torch.full((rows * self.ld + GUARD,), SENT, dtype=dtype, device=dev)
        self.t = self.flat[: rows * self.ld].view(rows, self.ld)
        self.v = self.t[:, :cols]
        self.v[...] = init.to(dev).to(dtype).view(rows, cols) if isinstance(init, torch.Tensor) else init

    def intact(self):
        ok = bool((self.flat[self.rows * self.ld:] == SENT).all()) and bool((self.t[:, self.cols:] == SENT).all())
        assert ok, "a write outside the output's extent (guard or pad columns changed)"
        return True


def hold(tag, got, ref, bnd):
    r = ratio(got, ref, bnd)
    print(f"tail/{tag} {r:.3f}")
    assert chk(r, 1.0, name=f"tail/{tag}"), f"tail/{tag}: worst |err| / bound {r:.3f}"


def bits(t):
    return t.contiguous().view(torch.int16)


def same_bits(a, b):
    return torch.equal(bits(a.cpu()), bits(b.cpu()))


# ============================================================================================ LayerNorm
def _ln_fwd(dev, x, rows, D, gm, bt, y16=None, y32=None, mean=None, rstd=None, in_group=0, in_stride=0, dtype16=0):
    call("devit_layernorm_fwd", x, rows, D, in_group, in_stride, gm, bt, T.LN_EPS, y16, y32, mean, rstd, dtype16)


@pytest.mark.parametrize("D,rows", T.ln_cases())
def test_layernorm_fwd(dev, D, rows):
    i = T.ln_inputs(D, rows)
    x, gm, bt = i["x"].to(dev), i["gamma"].to(dev), i["beta"].to(dev)
    ref, bnd = T.ln_fwd_bounds(i["x"], i["gamma"], i["beta"])
    tag = f"layernorm_fwd/D{D}_rows{rows}"
    y32, yb, mean, rstd = Out(dev, rows, D), Out(dev, rows, D, BF16), Out(dev, 1, rows), Out(dev, 1, rows)
    _ln_fwd(dev, x, rows, D, gm, bt, yb.t, y32.t, mean.t, rstd.t)
    assert y32.intact() and yb.intact() and mean.intact() and rstd.intact()
    hold(f"{tag}/y_f32", y32.v, ref["y"], bnd["y"])
    hold(f"{tag}/mean", mean.v[0], ref["mean"], bnd["mean"])
    hold(f"{tag}/rstd", rstd.v[0], ref["rstd"], bnd["rstd"])
    hold(f"{tag}/y_bf16", yb.v, ref["y"], stored16(bnd["y"], ref["y"]))
    assert same_bits(yb.v, y32.v.to(BF16)), "y_bf16 is one rounding of the y_f32 of the same launch"
    const = i["regime"] == 3          # a constant row: rstd = eps^-1/2, y = beta, within their bounds (held above); in plain terms too
    if bool(const.any()):
        assert float((rstd.v[0].cpu()[const] / T._f(T.LN_EPS) ** -0.5 - 1).abs().max()) < 1e-3
    if rows > 250:          # deliberate: the grid-capped case is there for the trip loop; the output variants below do not depend on the row count
        return
    # each output alone, mean / rstd NULL: the same bits
    y32b, ybb, yh = Out(dev, rows, D), Out(dev, rows, D, BF16), Out(dev, rows, D, F16)
    _ln_fwd(dev, x, rows, D, gm, bt, None, y32b.t)
    _ln_fwd(dev, x, rows, D, gm, bt, ybb.t, None)
    _ln_fwd(dev, x, rows, D, gm, bt, yh.t, None, dtype16=1)
    assert y32b.intact() and ybb.intact() and yh.intact()
    assert torch.equal(y32b.v, y32.v) and same_bits(ybb.v, yb.v)
    hold(f"{tag}/y_f16", yh.v, ref["y"], stored16(bnd["y"], ref["y"], f16=True))
    assert same_bits(yh.v, y32.v.to(F16)), "y in f16 is one rounding of y_f32"
    yh2, y32c = Out(dev, rows, D, F16), Out(dev, rows, D)
    _ln_fwd(dev, x, rows, D, gm, bt, yh2.t, y32c.t, dtype16=1)
    assert same_bits(yh2.v, yh.v) and torch.equal(y32c.v, y32.v) and yh2.intact() and y32c.intact()


@pytest.mark.parametrize("D", T.LN_BAD_DS)
def test_layernorm_refuses_width(dev, D):
    t = torch.zeros(4 * 1152, device=dev)
    refused("devit_layernorm_fwd", t, 2, D, 0, 0, t, t, T.LN_EPS, None, t, None, None, 0)
    refused("devit_layernorm_bwd", t, 1, t, 2, D, 0, 0, t, t, t, None, t, None, None, 0, t, t, None, 0, t, t.numel() * 4)


def _ln_bwd(dev, i, rows, D, mean, rstd, *, dy_f32, dres, dxb, colsum, rowscale, accumulate, x=None, dx_rows=None, in_group=0, in_stride=0):
    """one devit_layernorm_bwd call on guarded outputs -> dict of Out"""
    L = _L()
    dx_rows = rows if dx_rows is None else dx_rows
    o = dict(dx=Out(dev, dx_rows, D, init=SENT), dgamma=Out(dev, 1, D, init=i["dgamma0"] if accumulate else NAN),
             dbeta=Out(dev, 1, D, init=i["dbeta0"] if accumulate else NAN))
    if dxb:
        o["dxb"] = Out(dev, dx_rows, D, BF16, init=SENT)
    if colsum:
        o["colsum"] = Out(dev, 1, D, init=i["colsum0"] if accumulate else NAN)
    nws = L.load().devit_layernorm_bwd_workspace(rows, D)
    ws = Out(dev, 1, nws // 4)
    dy = i["dy"].to(dev) if dy_f32 else i["dy"].to(dev).to(BF16)
    call("devit_layernorm_bwd", dy, int(dy_f32), i["x"].to(dev) if x is None else x, rows, D, in_group, in_stride, mean, rstd, i["gamma"].to(dev),
         dres, o["dx"].t, o["dxb"].t if dxb else None, rowscale, i["rows_per_scale"], o["dgamma"].t, o["dbeta"].t,
         o["colsum"].t if colsum else None, int(accumulate), ws.t, nws)
    assert ws.intact() and all(v.intact() for v in o.values())
    return o


@pytest.mark.parametrize("D,rows", [c for c in T.ln_cases() if c[1] != T.LN_FWD_CAP_ROWS])
def test_layernorm_bwd(dev, D, rows):
    i = T.ln_inputs(D, rows)
    mean, rstd = torch.empty(rows, device=dev), torch.empty(rows, device=dev)
    y = torch.empty((rows, D), device=dev)
    _ln_fwd(dev, i["x"].to(dev), rows, D, i["gamma"].to(dev), i["beta"].to(dev), None, y, mean, rstd)
    tag = f"layernorm_bwd/D{D}_rows{rows}"
    rsc_rows = i["rowscale"][torch.arange(rows) // i["rows_per_scale"]]
    variants = [dict(name="bf16_dres_acc", dy_f32=False, dres=True, dxb=True, colsum=True, rowscale=True, accumulate=True),
                dict(name="f32_plain", dy_f32=True, dres=False, dxb=True, colsum=False, rowscale=False, accumulate=False),
                dict(name="f32_dres_nodxb", dy_f32=True, dres=True, dxb=False, colsum=False, rowscale=True, accumulate=False)]
    if rows > 250:          # deliberate: one variant (every optional output on) suffices for the grid-capped trip loop
        variants = variants[:1]
    for v in variants:
        dres = i["dres"] if v["dres"] else None
        g0, b0 = (i["dgamma0"], i["dbeta0"]) if v["accumulate"] else (None, None)
        ref, bnd = T.ln_bwd_bounds(i["x"], mean.cpu(), rstd.cpu(), i["gamma"], i["dy"], dres, g0, b0)
        o = _ln_bwd(dev, i, rows, D, mean, rstd, dy_f32=v["dy_f32"], dres=None if dres is None else dres.to(dev), dxb=v["dxb"],
                    colsum=v["colsum"], rowscale=i["rowscale"].to(dev) if v["rowscale"] else None, accumulate=v["accumulate"])
        for k in ("dx", "dgamma", "dbeta"):
            got = o[k].v if k == "dx" else o[k].v[0]
            hold(f"{tag}/{v['name']}/{k}", got, ref[k], bnd[k])
        if v["dxb"]:
            dx = o["dx"].v
            want = (dx * rsc_rows.to(dev)[:, None]).to(BF16) if v["rowscale"] else dx.to(BF16)
            assert same_bits(o["dxb"].v, want), "dx_bf16 == bf16(rowscale * dx) from the returned dx"
        if v["colsum"]:
            cs, ecs = T.ln_colsum_bounds(o["dxb"].v.cpu(), i["colsum0"] if v["accumulate"] else None)
            hold(f"{tag}/{v['name']}/dx_bf16_colsum", o["colsum"].v[0], cs, ecs)


@pytest.mark.parametrize("D", [192, 384])
def test_layernorm_row_groups(dev, D):
    """in_group = 2, in_stride = T: logical row r reads physical row (r / 2) T + r % 2; every other row of x (and of dres) holds NaN; the backward
    writes dx (and dx_bf16) at the physical rows only"""
    B, Tk = 5, 7
    rows = 2 * B
    i = T.ln_inputs(D, rows)
    phys = torch.tensor([(r // 2) * Tk + r % 2 for r in range(rows)])
    xp = torch.full((B * Tk, D), NAN)
    xp[phys] = i["x"]
    dresp = torch.full((B * Tk, D), NAN)
    dresp[phys] = i["dres"]
    x = xp.to(dev)
    ref, bnd = T.ln_fwd_bounds(i["x"], i["gamma"], i["beta"])
    y32, mean, rstd = Out(dev, rows, D), Out(dev, 1, rows), Out(dev, 1, rows)
    _ln_fwd(dev, x, rows, D, i["gamma"].to(dev), i["beta"].to(dev), None, y32.t, mean.t, rstd.t, in_group=2, in_stride=Tk)
    assert y32.intact() and mean.intact() and rstd.intact()
    tag = f"layernorm_fwd/in_group_D{D}"
    hold(f"{tag}/y_f32", y32.v, ref["y"], bnd["y"])
    hold(f"{tag}/mean", mean.v[0], ref["mean"], bnd["mean"])
    hold(f"{tag}/rstd", rstd.v[0], ref["rstd"], bnd["rstd"])
    i["rows_per_scale"] = Tk          # the scale of dx_bf16 goes by the PHYSICAL row: one per image
    rscale = torch.tensor([0.5, 2.0, 0.0, 1.0, 0.25])
    m, r = mean.v[0].contiguous(), rstd.v[0].contiguous()
    bref, bbnd = T.ln_bwd_bounds(i["x"], m.cpu(), r.cpu(), i["gamma"], i["dy"], i["dres"], i["dgamma0"], i["dbeta0"])
    o = _ln_bwd(dev, i, rows, D, m, r, dy_f32=False, dres=dresp.to(dev), dxb=True, colsum=True, rowscale=rscale.to(dev), accumulate=True, x=x,
                dx_rows=B * Tk, in_group=2, in_stride=Tk)
    tag = f"layernorm_bwd/in_group_D{D}"
    hold(f"{tag}/dx", o["dx"].v[phys.to(dev)], bref["dx"], bbnd["dx"])
    hold(f"{tag}/dgamma", o["dgamma"].v[0], bref["dgamma"], bbnd["dgamma"])
    hold(f"{tag}/dbeta", o["dbeta"].v[0], bref["dbeta"], bbnd["dbeta"])
    other = torch.ones(B * Tk, dtype=torch.bool)
    other[phys] = False
    assert bool((o["dx"].v[other.to(dev)] == SENT).all()) and bool((o["dxb"].v[other.to(dev)] == SENT).all()), "rows outside the map were written"
    want = (o["dx"].v[phys.to(dev)] * rscale[phys // Tk].to(dev)[:, None]).to(BF16)
    assert same_bits(o["dxb"].v[phys.to(dev)], want)
    cs, ecs = T.ln_colsum_bounds(o["dxb"].v[phys.to(dev)].cpu(), i["colsum0"])
    hold(f"{tag}/dx_bf16_colsum", o["colsum"].v[0], cs, ecs)


# ============================================================================================ elementwise.hip
@pytest.mark.parametrize("c", T.sgemm_cases(), ids=lambda c: f"K{c['K']}-{c['M']}x{c['N']}-{c['form']}-{'int' if c['ints'] else 'rnd'}")
def test_sgemm_small(dev, c):
    i = T.sgemm_inputs(c)
    M, N, K = c["M"], c["N"], c["K"]
    A, B = i["A"], i["B"]
    if c["form"] == "token":            # the class-token view of a [M][2][K] buffer (ops.HeadsFn): sam = 2 K; the other token holds NaN
        buf = torch.full((M, 2, K), NAN)
        buf[:, 1] = A
        buf = buf.to(dev)
        a_arg, sam, sak = buf[:, 1], 2 * K, 1
        b_arg, sbn, sbk = B.to(dev), K, 1
    elif c["form"] == "b_transposed":   # B stored [K][N]
        a_arg, sam, sak = A.to(dev), K, 1
        b_arg, sbn, sbk = B.t().contiguous().to(dev), 1, N
    else:                               # A stored [K][M]
        a_arg, sam, sak = A.t().contiguous().to(dev), 1, M
        b_arg, sbn, sbk = B.to(dev), K, 1
    out = Out(dev, M, N, ld=N + 3, init=i["C0"] if c["accumulate"] else NAN)
    bias = None if i["bias"] is None else i["bias"].to(dev)
    call("devit_sgemm_small", a_arg, sam, sak, b_arg, sbn, sbk, bias, out.t, N + 3, M, N, K, c["alpha"], int(c["accumulate"]))
    assert out.intact()
    ref, bnd = T.sgemm_bounds(A, B, i["bias"], i["C0"], c["alpha"], c["accumulate"])
    if c["ints"]:
        assert torch.equal(out.v.cpu().to(F64), ref), "small integers: every partial sum is exact, whatever the order"
    else:
        hold(f"sgemm_small/K{K}_{M}x{N}_{c['form']}/C", out.v, ref, bnd)


@pytest.mark.parametrize("M,N,grp,skip,acc", T.colsum_cases())
def test_colsum_bf16(dev, M, N, grp, skip, acc):
    L = _L()
    i = T.colsum_inputs(M, N, grp, skip)
    y = i["y"].to(dev).to(BF16)
    out = Out(dev, 1, N, init=i["out0"] if acc else NAN)
    nws = L.load().devit_colsum_workspace(M, N)
    ws = Out(dev, 1, nws // 4)
    call("devit_colsum_bf16", y, M, N, N + 8, grp, skip, out.t, int(acc), ws.t, nws)
    assert out.intact() and ws.intact()
    assert torch.equal(out.v[0].cpu().to(F64), T.colsum_ref(i["y"], M, N, grp, skip, i["out0"] if acc else None))


def test_colsum_bf16_refusals(dev):
    y = torch.zeros((600, 24), dtype=BF16, device=dev)
    out, ws = torch.zeros(16, device=dev), torch.zeros(64 * 16, device=dev)
    refused("devit_colsum_bf16", y, 600, 12, 24, 0, 0, out, 0, ws, ws.numel() * 4)
    refused("devit_colsum_bf16", y, 600, 16, 24, 0, 0, out, 0, ws, 63 * 16 * 4)


@pytest.mark.parametrize("M,N", [(7, 5), (300, 257)])
def test_fp32_helpers(dev, M, N):
    """devit_colsum_f32 (exact integers, ld > N), devit_scale_rows_f32 (one rounded product per element: bit-exact)"""
    g = T.gen("f32help", M, N)
    y = torch.full((M, N + 3), NAN)
    y[:, :N] = T.randint(g, -3, 3, M, N)
    out0 = T.randint(g, -5, 5, N)
    for acc in (False, True):
        out = Out(dev, 1, N, init=out0 if acc else NAN)
        call("devit_colsum_f32", y.to(dev), M, N, N + 3, out.t, int(acc))
        assert out.intact() and torch.equal(out.v[0].cpu().to(F64), y[:, :N].to(F64).sum(0) + (out0.to(F64) if acc else 0))
    src = T.randn(g, M, N)
    rps = 3
    rs = torch.tensor([T.ROWSCALE_MIX[k % 4] for k in range((M + rps - 1) // rps)])
    for rowscale in (None, rs):
        dst = Out(dev, M, N)
        call("devit_scale_rows_f32", src.to(dev), dst.t, None if rowscale is None else rowscale.to(dev), rps, M, N)
        want = src if rowscale is None else src * rowscale[torch.arange(M) // rps][:, None]
        assert dst.intact() and torch.equal(dst.v.cpu(), want)


@pytest.mark.parametrize("B", [1, 2])
def test_im2row_f32(dev, B):
    img = T.randn(T.gen("im2row", B), B, 3, 224, 224)
    rows = Out(dev, B * 196, 768)
    call("devit_im2row_f32", img.to(dev), rows.t, B)
    want = img.reshape(B, 3, 14, 16, 14, 16).permute(0, 2, 4, 1, 3, 5).reshape(B * 196, 768)
    assert rows.intact() and torch.equal(rows.v.cpu(), want)


@pytest.mark.parametrize("B,Tk,D,ntok", [(1, 7, 260, 2), (5, 7, 260, 2), (64, 7, 260, 2), (67, 7, 260, 2), (1, 6, 4, 1), (5, 6, 4, 1), (64, 6, 4, 1),
                                         (67, 6, 4, 1), (5, 198, 384, 2)])
def test_embed_bwd(dev, B, Tk, D, ntok):
    dx = T.randint(T.gen("embed_bwd", B, Tk, D), -3, 3, B, Tk, D)
    for with16 in (True, False):
        dpos, dcls, dbias = Out(dev, Tk, D), Out(dev, 1, D), Out(dev, 1, D)
        ddist = Out(dev, 1, D) if ntok == 2 else None
        d16 = Out(dev, B * Tk, D, BF16) if with16 else None
        call("devit_embed_bwd", dx.to(dev), B, Tk, D, ntok, dpos.t, dcls.t, ddist.t if ddist else None, dbias.t, d16.t if d16 else None, 0)
        want = dx.to(F64).sum(0)
        assert dpos.intact() and dcls.intact() and dbias.intact() and (ddist is None or ddist.intact())
        assert torch.equal(dpos.v.cpu().to(F64), want)
        assert torch.equal(dbias.v[0].cpu().to(F64), want[ntok:].sum(0))
        assert torch.equal(dcls.v[0], dpos.v[0]) and (ddist is None or torch.equal(ddist.v[0], dpos.v[1]))
        if d16:
            assert d16.intact() and same_bits(d16.v, dx.view(B * Tk, D).to(BF16))
    t = torch.zeros(Tk * D, device=dev)
    refused("devit_embed_bwd", dx.to(dev), B, Tk, D, ntok, t, t, t, t, None, 1)
    if ntok == 2:
        refused("devit_embed_bwd", dx.to(dev), B, Tk, D, 2, t, t, None, t, None, 0)


@pytest.mark.parametrize("B,Tk,D", [(3, 7, 260), (2, 5, 4)])
def test_embed_tokens(dev, B, Tk, D):
    g = T.gen("embed_tokens", B, Tk, D)
    cls, dist, pos = T.randn(g, D), T.randn(g, D), T.randn(g, Tk, D)
    for with_dist in (True, False):
        ntok = 2 if with_dist else 1
        x = Out(dev, B * Tk, D, init=SENT)
        call("devit_embed_tokens", cls.to(dev), dist.to(dev) if with_dist else None, pos.to(dev), x.t, B, Tk, D)
        got = x.v.cpu().view(B, Tk, D)
        assert x.intact() and torch.equal(got[:, 0], (cls + pos[0]).expand(B, D))
        if with_dist:
            assert torch.equal(got[:, 1], (dist + pos[1]).expand(B, D))
        assert bool((got[:, ntok:] == SENT).all()), "rows t >= ntok belong to the patch GEMM"


@pytest.mark.parametrize("M,D,rowscale", [(9, 4, False), (9, 4, True), (9, 260, False), (9, 260, True), (16400, 260, True)])
def test_scale_cast_bf16(dev, M, D, rowscale):
    """bf16(src * scale): one fp32 product, one rounding -- bit-exact; 16400 x 260 lies past the grid cap (M D > 4096 * 256 * 4)"""
    src = T.randn(T.gen("scale_cast", M, D), M, D)
    rps = 3 if M < 100 else 4100
    rs = torch.tensor([T.ROWSCALE_MIX[k % 4] for k in range((M + rps - 1) // rps)])
    dst = Out(dev, M, D, BF16)
    call("devit_scale_cast_bf16", src.to(dev), dst.t, rs.to(dev) if rowscale else None, rps, M, D)
    want = (src * rs[torch.arange(M) // rps][:, None] if rowscale else src).to(BF16)
    assert dst.intact() and same_bits(dst.v, want)


def test_scale_cast_bf16_refuses_width(dev):
    t = torch.zeros(64, device=dev)
    refused("devit_scale_cast_bf16", t, t, None, 1, 2, 6)


def _cast_specials():
    """round-to-even ties of both types, +-inf, values that round up to inf, f16-subnormal magnitudes (and the tie at half the smallest one)"""
    v = [1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -8), 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, math.inf, -math.inf, 3.4e38, -3.4e38,
         65519.0, 65520.0, -65520.0, 1e5, 0.0, -0.0, 2.0 ** -14, 2.0 ** -15, 1e-5, -3e-6, 6e-8, 2.0 ** -24, 2.0 ** -25, 1.5 * 2.0 ** -24, -2.0 ** -25,
         2.0 ** -26, 1e-30]
    return torch.tensor(v, dtype=F32)


@pytest.mark.parametrize("n", [1, 7, 8, 9, 2048 * 256 * 8 + 5])
@pytest.mark.parametrize("f16", [False, True])
def test_cast_bf16(dev, n, f16):
    sp = _cast_specials()
    src = torch.cat([sp.roll(-n % sp.numel()), T.randn(T.gen("cast", n), max(0, n - sp.numel())) * 3])[:n]
    if n > 100:
        src[-5:] = sp[:5]          # the tail elements (n & 7) take the scalar path
    dt = F16 if f16 else BF16
    dst = Out(dev, 1, n, dt)
    buf = torch.empty(n + 8, device=dev)
    buf[:n] = src.to(dev)
    call("devit_cast_bf16", buf, dst.t, n, int(f16))
    assert dst.intact()
    got, want = dst.v[0].cpu(), src.to(dt)
    bad = bits(got) != bits(want)
    assert not bool(bad.any()), f"cast to {dt}: {[(float(a), float(b), float(c)) for a, b, c in zip(src[bad][:8], got[bad][:8], want[bad][:8])]}"


def test_cast_bf16_refuses_misaligned(dev):
    src, dst = torch.zeros(64, device=dev), torch.zeros(64, dtype=BF16, device=dev)
    refused("devit_cast_bf16", src[1:], dst, 8, 0)
    refused("devit_cast_bf16", src, dst[1:], 8, 0)


@pytest.mark.parametrize("B", [1, 5])
def test_mix_targets(dev, B):
    """lam * smooth(y) + (1 - lam) * smooth(y.flip(0)) with each product and the sum rounded apart (the kernel's contract(off)): torch fp32 does that"""
    Cn, lam, sm = 1000, 0.3, 0.1
    labels = torch.randint(0, Cn, (B,), generator=T.gen("mix_targets", B))
    out = Out(dev, B, Cn)
    call("devit_mix_targets", labels.to(dev), out.t, B, Cn, C.c_double(lam), C.c_double(sm))
    off, on = torch.tensor(sm / Cn, dtype=F32), torch.tensor(1.0 - sm + sm / Cn, dtype=F32)
    hot = lambda y: torch.where(torch.arange(Cn)[None, :] == y[:, None], on, off)
    want = hot(labels) * torch.tensor(lam, dtype=F32) + hot(labels.flip(0)) * torch.tensor(1.0 - lam, dtype=F32)
    assert out.intact() and torch.equal(out.v.cpu(), want)


# ============================================================================================ losses.hip
@pytest.mark.parametrize("B", T.CLS_BS)
@pytest.mark.parametrize("Cn", T.CLS_CS)
def test_cls_distill_loss(dev, B, Cn):
    for (b, c, kind, alpha, tau, variant) in [k for k in T.cls_cases() if k[0] == B and k[1] == Cn]:
        i = T.cls_inputs(B, Cn, variant)
        ref, bnd = T.cls_bounds(i["lo"], i["lk"], i["lt"], i["y"], kind, alpha, tau)
        loss3, dlo, dlk = Out(dev, 1, 3), Out(dev, B, Cn), Out(dev, B, Cn)
        lt = None if (kind == T.KIND_NONE and variant == "std3") else i["lt"].to(dev)
        call("devit_cls_distill_loss", i["lo"].to(dev), i["lk"].to(dev), lt, i["y"].to(dev), B, Cn, kind, alpha, tau, loss3.t, dlo.t, dlk.t)
        assert loss3.intact() and dlo.intact() and dlk.intact()
        tag = f"cls_distill_loss/B{B}_C{Cn}_kind{kind}_a{alpha}_t{tau}_{variant}"
        hold(f"{tag}/loss3", loss3.v[0], ref["loss3"], bnd["loss3"])
        hold(f"{tag}/dlogits", dlo.v, ref["dlo"], bnd["dlo"])
        hold(f"{tag}/dlogits_kd", dlk.v, ref["dlk"], bnd["dlk"])
        if kind == T.KIND_NONE:
            assert not bool(dlk.v.any()), "dlogits_kd == 0 for kind none"


def test_cls_distill_loss_refuses_1025(dev):
    t = torch.zeros(2 * 1025, device=dev)
    refused("devit_cls_distill_loss", t, t, t, t, 2, 1025, 1, 0.5, 1.0, t, t, t)


@pytest.mark.parametrize("n", T.MSE_NS)
def test_token_mse(dev, n):
    i = T.mse_inputs(n)
    a, b = i["a"].to(dev), i["b"].to(dev)
    for acc, with_da in ((False, True), (True, True), (False, False)):
        loss, da = Out(dev, 1, 1, init=i["loss0"] if acc else NAN), Out(dev, 1, n)
        call("devit_token_mse", a, b, n, loss.t, da.t if with_da else None, int(acc))
        ref, bnd = T.mse_bounds(i["a"], i["b"], i["loss0"] if acc else None)
        assert loss.intact() and da.intact()
        hold(f"token_mse/n{n}_acc{int(acc)}_da{int(with_da)}/loss", loss.v[0, 0], ref["loss"], bnd["loss"])
        if with_da:
            hold(f"token_mse/n{n}_acc{int(acc)}/da", da.v[0], ref["da"], bnd["da"])
        else:
            assert bool(torch.isnan(da.v).all())


def _padded_gram(g, ldr, dev):
    B, N, _ = g.shape
    p = torch.full((B, ldr, ldr), NAN)
    p[:, :N, :N] = g
    return p.to(dev)


@pytest.mark.parametrize("B,N,hd_t,hd_s,scale", T.rel_cases())
def test_relation_stats_and_grad(dev, B, N, hd_t, hd_s, scale):
    i = T.rel_inputs(B, N, hd_t, hd_s, scale)
    ref, bnd = T.rel_stats_bounds(i["gram_t"], i["gram_s"], hd_t, hd_s)
    tag = f"relation/B{B}_N{N}_hd{hd_t}_{hd_s}_{scale}"
    ldr = 200 if N <= 200 else 256
    lt, ls, kl, loss = Out(dev, B, N), Out(dev, B, N), Out(dev, B, N), Out(dev, 1, 1)
    call("devit_relation_stats", _padded_gram(i["gram_t"], ldr, dev), _padded_gram(i["gram_s"], ldr, dev), B, N, ldr, hd_t, hd_s, lt.t, ls.t,
         kl.t, loss.t)
    assert lt.intact() and ls.intact() and kl.intact() and loss.intact()
    hold(f"{tag}/stats/lse_t", lt.v, ref["lse_t"], bnd["lse_t"])
    hold(f"{tag}/stats/lse_s", ls.v, ref["lse_s"], bnd["lse_s"])
    hold(f"{tag}/stats/row_kl", kl.v, ref["row_kl"], bnd["row_kl"])
    hold(f"{tag}/stats/loss", loss.v[0, 0], ref["loss"], bnd["loss"])
    gt, gs = _padded_gram(i["gram_t"], 256, dev), _padded_gram(i["gram_s"], 256, dev)
    lse_t, lse_s = lt.v.contiguous(), ls.v.contiguous()
    inside = torch.zeros((256, 256), dtype=torch.bool)
    inside[:N, :N] = True
    for up, f32_out in ((None, False), (0.37, True), (0.37, False), (None, True)):
        S = Out(dev, B * 256, 256, F32 if f32_out else BF16)
        upt = None if up is None else torch.tensor([up], device=dev)
        call("devit_relation_grad", gt, gs, lse_t, lse_s, upt, B, N, 256, hd_t, hd_s, S.t, int(f32_out))
        assert S.intact()
        want, eS = T.rel_grad_bounds(i["gram_t"], i["gram_s"], lse_t.cpu(), lse_s.cpu(), None if up is None else T._f(up), hd_t, hd_s, not f32_out)
        got = S.v.cpu().view(B, 256, 256)
        hold(f"{tag}/grad/up{up}_{'f32' if f32_out else 'bf16'}/S", got[:, :N, :N], want, eS)
        assert not bool(got[:, ~inside].any()), "S is exactly 0 outside N x N"


# ============================================================================================ index copies (shrink.hip)
@pytest.mark.parametrize("blocks_per_job", [1, 64])
def test_index_copy(dev, blocks_per_job):
    """one call: gathers of rows and of columns in both element sizes, both adds, and a transpose; idx holds -1 (padding units)"""
    L = _L()
    g = T.gen("index_copy", blocks_per_job)
    rows, cols, Rm, Cm = 37, 29, 50, 41            # compact extent; the masters have Rm rows (row maps) / Cm columns (column maps)
    ridx = torch.randperm(Rm, generator=g)[:rows].to(torch.int32)
    cidx = torch.randperm(Cm, generator=g)[:cols].to(torch.int32)
    ridx[[3, rows - 1]] = -1
    cidx[[0, 7]] = -1
    rd, cd = ridx.to(dev), cidx.to(dev)
    jobs, checks, alive = [], [], []

    def job(src, dst, idx, r, c, sld, dld, mode, elem):
        alive.extend((src, dst))          # the table holds raw pointers: the tensors must outlive the launch
        jobs.append(L.IndexJob(src.data_ptr(), dst.data_ptr(), 0 if idx is None else idx.data_ptr(), r, c, sld, dld, mode, elem))

    for dt, elem in ((BF16, 2), (F32, 4)):
        # mode 0: dst[i][c] = src[ridx[i]][c]
        src = T.randint(g, -100, 100, Rm, cols + 3).to(dt).to(dev)
        dst = Out(dev, rows, cols, dt, ld=cols + 5, init=SENT)
        job(src, dst.t, rd, rows, cols, cols + 3, cols + 5, 0, elem)
        want = torch.full((rows, cols), SENT, dtype=dt)
        keep = ridx >= 0
        want[keep] = src.cpu()[ridx[keep].long(), :cols]
        checks.append((dst, want, "gather rows"))
        # mode 1: dst[r][j] = src[r][cidx[j]]
        src = T.randint(g, -100, 100, rows, Cm + 2).to(dt).to(dev)
        dst = Out(dev, rows, cols, dt, ld=cols + 1, init=SENT)
        job(src, dst.t, cd, rows, cols, Cm + 2, cols + 1, 1, elem)
        want = torch.full((rows, cols), SENT, dtype=dt)
        keep = cidx >= 0
        want[:, keep] = src.cpu()[:rows, cidx[keep].long()]
        checks.append((dst, want, "gather columns"))
    adds = []
    for mode in (2, 3):
        src = Out(dev, rows, cols, F32, ld=cols + 2, init=T.randn(g, rows, cols))
        mr, mc = (Rm, cols) if mode == 2 else (rows, Cm)
        d0 = T.randn(g, mr, mc)
        dst = Out(dev, mr, mc, F32, ld=mc + 4, init=d0)
        s0 = src.v.cpu().clone()
        job(src.t, dst.t, rd if mode == 2 else cd, rows, cols, cols + 2, mc + 4, mode, 4)
        want = d0.clone()
        if mode == 2:
            keep = ridx >= 0
            want[ridx[keep].long()] += s0[keep]
        else:
            keep = cidx >= 0
            want[:, cidx[keep].long()] += s0[:, keep]
        adds.append((src, dst, want))
    tsrc = T.randint(g, -100, 100, 70, 33 + 1).to(BF16).to(dev)
    tdst = Out(dev, 33, 70, BF16, ld=72, init=SENT)
    job(tsrc, tdst.t, None, 70, 33, 34, 72, 4, 2)
    arr = (L.IndexJob * len(jobs))(*jobs)
    table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev)
    call("devit_index_copy", table, len(jobs), blocks_per_job)
    for dst, want, what in checks:
        assert dst.intact(), what
        assert same_bits(dst.v, want) if dst.v.element_size() == 2 else torch.equal(dst.v.cpu(), want), what
    for src, dst, want in adds:
        assert src.intact() and dst.intact()
        assert torch.equal(dst.v.cpu(), want), "dst + src in one fp32 add; the rest of dst untouched"
        assert not bool(src.v.any()), "the compact accumulator is zeroed everywhere, padding units included"
    assert tdst.intact() and same_bits(tdst.v, tsrc[:, :33].t())
    refused("devit_index_copy", table, 0, 1)
    refused("devit_index_copy", table, len(jobs), 4097)


# ============================================================================================ exact-fp32 companions (sgemm.hip)
@pytest.mark.parametrize("rows", T.SOFTMAX_ROWS)
@pytest.mark.parametrize("ncols", T.SOFTMAX_COLS)
def test_softmax_rows_f32(dev, rows, ncols):
    i = T.softmax_inputs(rows, ncols)
    ld = ncols + 3
    ref, bnd = T.softmax_bounds(i["S"], i["scale"])
    tag = f"softmax_rows_f32/{rows}x{ncols}"

    def padded(v):
        t = torch.full((rows, ld), NAN)
        t[:, :ncols] = v
        return t.to(dev)

    P = None
    for with_lse in (True, False):
        S = padded(i["S"])
        lse = Out(dev, 1, rows)
        call("devit_softmax_rows_f32", S, rows, ncols, ld, i["scale"], lse.t if with_lse else None)
        assert bool(torch.isnan(S[:, ncols:]).all()) and lse.intact()
        if with_lse:
            hold(f"{tag}/P", S[:, :ncols], ref["P"], bnd["P"])
            hold(f"{tag}/lse", lse.v[0], ref["lse"], bnd["lse"])
            P = S
        else:
            assert torch.equal(S[:, :ncols], P[:, :ncols])
    dP = padded(i["dP"])
    call("devit_softmax_bwd_rows_f32", P, dP, rows, ncols, ld, i["scale"])
    dS, edS = T.softmax_bwd_bounds(P[:, :ncols].cpu(), i["dP"], i["scale"])
    assert bool(torch.isnan(dP[:, ncols:]).all())
    hold(f"softmax_bwd_rows_f32/{rows}x{ncols}/dS", dP[:, :ncols], dS, edS)


def _sgemm(dev, A, sam, sak, B, sbn, sbk, M, N, K, out, ldc, kind=None, **kw):
    from devit_amd import ops_f32
    L = _L()
    ops_f32.sgemm(A, sam, sak, B, sbn, sbk, M, N, K, out=out, ldc=ldc, kind=L.EPI_STORE_F32 if kind is None else kind, **kw)


@pytest.mark.parametrize("M,N,K", [(1, 1, 1), (63, 65, 17), (130, 64, 40)])
def test_gemm_f32_store(dev, M, N, K):
    """STORE_F32: exact integers in every addressing form (plain, transposed B, k_group / k_skip with NaN in the skipped k, batched with outer / inner
    strides and batch_scale, accumulate, m_valid), then one random case under the bound"""
    g = T.gen("gemm_f32", M, N, K)
    A, B, bias, C0 = T.randint(g, -3, 3, M, K), T.randint(g, -3, 3, N, K), T.randint(g, -3, 3, N), T.randint(g, -5, 5, M, N)
    ld = N + 3
    want = A.to(F64) @ B.to(F64).t()
    out = Out(dev, M, N, ld=ld)
    _sgemm(dev, A.to(dev), K, 1, B.to(dev), K, 1, M, N, K, out.t, ld, bias=bias.to(dev))
    assert out.intact() and torch.equal(out.v.cpu().to(F64), want + bias.to(F64))
    out = Out(dev, M, N, ld=ld, init=C0)            # transposed B ([K][N]), alpha, accumulate
    _sgemm(dev, A.to(dev), K, 1, B.t().contiguous().to(dev), 1, N, M, N, K, out.t, ld, alpha=2.0, accumulate=True)
    assert out.intact() and torch.equal(out.v.cpu().to(F64), 2 * want + C0.to(F64))
    if K > 1:                                       # physical k of A = k + skip (k / group + 1): the skipped k hold NaN
        grp, skip = 5, 2
        pk = torch.tensor([k + skip * (k // grp + 1) for k in range(K)])
        Ap = torch.full((M, int(pk[-1]) + 1), NAN)
        Ap[:, pk] = A
        out = Out(dev, M, N, ld=ld)
        _sgemm(dev, Ap.to(dev), Ap.shape[1], 1, B.to(dev), K, 1, M, N, K, out.t, ld, k_group=grp, k_skip=skip)
        assert out.intact() and torch.equal(out.v.cpu().to(F64), want)
        mv = M - 2                                  # m_valid: the rows behind it keep the sentinel
        out = Out(dev, M, N, ld=ld, init=SENT)
        _sgemm(dev, A.to(dev), K, 1, B.to(dev), K, 1, M, N, K, out.t, ld, m_valid=mv)
        assert out.intact() and torch.equal(out.v[:mv].cpu().to(F64), want[:mv]) and bool((out.v[mv:] == SENT).all())
    # batch = 4 = 2 outer x 2 inner; A [zo][zi][M][K], B [zi][zo][N][K] (the strides say so), batch_scale by the inner index
    Ab, Bb = T.randint(g, -3, 3, 2, 2, M, K), T.randint(g, -3, 3, 2, 2, N, K)
    bs = torch.tensor([2.0, -1.0])
    out = Out(dev, 4 * M, N, ld=ld)
    _sgemm(dev, Ab.to(dev), K, 1, Bb.to(dev), K, 1, M, N, K, out.t, ld, batch=4, batch_inner=2, a_bo=2 * M * K, a_bi=M * K, b_bo=N * K, b_bi=2 * N * K,
           c_bo=2 * M * ld, c_bi=M * ld, batch_scale=bs.to(dev))
    wantb = torch.stack([torch.stack([bs[zi].to(F64) * (Ab[zo, zi].to(F64) @ Bb[zi, zo].to(F64).t()) for zi in range(2)]) for zo in range(2)])
    assert out.intact() and torch.equal(out.v.cpu().to(F64).reshape(2, 2, M, N), wantb)
    Ar, Br, br_ = T.randn(g, M, K), T.randn(g, N, K), T.randn(g, N)
    out = Out(dev, M, N, ld=ld)
    _sgemm(dev, Ar.to(dev), K, 1, Br.to(dev), K, 1, M, N, K, out.t, ld, bias=br_.to(dev), alpha=0.5)
    ref = 0.5 * (Ar.to(F64) @ Br.to(F64).t()) + br_.to(F64)
    bnd = T.gemm_f32_bound(Ar.to(F64).abs() @ Br.to(F64).abs().t(), 0.5, br_.to(F64).abs(), K)
    assert out.intact()
    hold(f"gemm_f32/store_{M}x{N}x{K}/C", out.v, ref, bnd)


def test_gemm_f32_epilogues(dev):
    """GELU, DGELU, RESIDUAL and PATCH in their fp32 flavours at (63, 65, 17) against float64"""
    L = _L()
    M, N, K = 63, 65, 17
    g = T.gen("gemm_f32_epi")
    A, B, bias = T.randn(g, M, K) * 0.5, T.randn(g, N, K) * 0.5, T.randn(g, N) * 0.2
    cs = 1 + 0.1 * T.randn(g, N)
    v = A.to(F64) @ B.to(F64).t() + bias.to(F64)
    e_v = T.gemm_f32_bound(A.to(F64).abs() @ B.to(F64).abs().t(), 1.0, bias.to(F64).abs(), K)
    Ad, Bd, bd, csd = A.to(dev), B.to(dev), bias.to(dev), cs.to(dev)
    c64 = cs.to(F64)
    out, aux = Out(dev, M, N), Out(dev, M, N)
    _sgemm(dev, Ad, K, 1, Bd, K, 1, M, N, K, out.t, N, kind=L.EPI_GELU_BF16, bias=bd, colscale=csd, aux=aux.t)
    assert out.intact() and aux.intact()
    hold("gemm_f32/gelu/aux", aux.v, v, e_v)
    ge = T.gelu64(v) * c64
    hold("gemm_f32/gelu/out", out.v, ge, T.gelu_bound(v, e_v) * c64.abs() + T.U * ge.abs())
    # DGELU: out = (acc + bias) * colscale * gelu'(aux_in)
    pre = T.randn(g, M, N) * 1.5
    out = Out(dev, M, N)
    _sgemm(dev, Ad, K, 1, Bd, K, 1, M, N, K, out.t, N, kind=L.EPI_DGELU_BF16, bias=bd, colscale=csd, aux_in=pre.to(dev))
    dg = T.dgelu64(pre.to(F64))
    ref = v * c64 * dg
    assert out.intact()
    hold("gemm_f32/dgelu/out", out.v, ref, (v * c64).abs() * T.dgelu_bound(pre.to(F64)) + dg.abs() * c64.abs() * e_v + 2 * T.U * ref.abs())
    # RESIDUAL: out = res + rowscale[m / rows_per_scale] * (acc + bias); aux = acc + bias
    res, rs = T.randn(g, M, N), torch.tensor([0.5, 0.0, 2.0])
    rsm = rs[torch.arange(M) // 21].to(F64)[:, None]
    out, aux = Out(dev, M, N), Out(dev, M, N)
    _sgemm(dev, Ad, K, 1, Bd, K, 1, M, N, K, out.t, N, kind=L.EPI_RESIDUAL_F32, bias=bd, res=res.to(dev), rowscale=rs.to(dev), rows_per_scale=21,
           aux=aux.t)
    ref = res.to(F64) + rsm * v
    assert out.intact() and aux.intact()
    hold("gemm_f32/residual/aux", aux.v, v, e_v)
    hold("gemm_f32/residual/out", out.v, ref, rsm.abs() * e_v + T.U * ((rsm * v).abs() + ref.abs()))
    # PATCH: row m = (b, t) of 3 images x 21 patch tokens goes to row b (21 + 2) + 2 + t, plus pos[2 + t]; the token rows keep the sentinel
    pos = T.randn(g, 23, N)
    out = Out(dev, 3 * 23, N, init=SENT)
    _sgemm(dev, Ad, K, 1, Bd, K, 1, M, N, K, out.t, N, kind=L.EPI_PATCH_F32, bias=bd, pos=pos.to(dev), patch_tokens=21, extra_tokens=2)
    got = out.v.cpu().view(3, 23, N)
    ref = v.view(3, 21, N) + pos.to(F64)[2:]
    assert out.intact() and bool((got[:, :2] == SENT).all())
    hold("gemm_f32/patch/out", got[:, 2:], ref, e_v.view(3, 21, N) + T.U * ref.abs())
