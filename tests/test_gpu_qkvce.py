"""cal_qkv_loss / cal_qkv_loss2 / soft_cross_entropy on the MI355X (csrc/qkvce.hip): the kernels per element against the float64 restatement inside the
bounds of tests/_qkvce_model.py, what they may and may not write, the public functions on packed and generic inputs, every refusal, and one engine step
with both weights on."""
import argparse
import json
import os

import numpy as np
import pytest
import torch

import _imgsize_model as IM
import _qkvce_model as QM
from conftest import chk
from oracle import devit_oracle as O
from test_gpu_hid import one_k_slice, step_setup
from test_gpu_tail import Out, call

pytestmark = pytest.mark.gpu
F32, F64, BF16, F16 = torch.float32, torch.float64, torch.bfloat16, torch.float16
GS, GT = O.GEOMETRY["dedeit"], O.GEOMETRY["deit_base_distilled_patch16_224"]
LAYOUT = {"view": 0, "tokens": 1}
MODES = [(cross, layout) for cross in (0, 1) for layout in ("view", "tokens")]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from devit_amd import _lib
    _lib.require_device(torch.zeros(1, device="cuda"))
    return torch.device("cuda")


def hold(tag, got, ref, bnd):
    r = QM.ratio(got, ref, bnd)
    print(f"qkvce/{tag} {r:.3f}")
    assert chk(r, 1.0, name=f"qkvce/{tag}"), f"qkvce/{tag}: worst |err| / bound {r:.3f}"


def packed(x, dtype, dev, behind=0.0, extra=40, pad=0):
    """[B N + extra rows][3 D + pad] 16-bit buffer holding x [B, N, 3 D] in its first rows and columns; everything else is `behind`"""
    B, N, W = x.shape
    buf = torch.full((B * N + extra, W + pad), behind, dtype=dtype, device=dev)
    buf[: B * N, :W] = x.reshape(B * N, W).to(dev).to(dtype)
    return buf


def run_fwd(dev, s_buf, t_buf, B, N, Ds, Dt, cross, layout, layers=1):
    P = 9 if cross else 3
    terms, S, loss = Out(dev, P, B * N), Out(dev, P * B * 208, 224, BF16), Out(dev, 1, 1)
    call("devit_qkv_pair_fwd", s_buf, t_buf, B, N, Ds, Dt, s_buf.stride(0), t_buf.stride(0), 64, 64, int(t_buf.dtype == F16), cross, LAYOUT[layout],
         layers, terms.t, S.t, loss.t)
    assert terms.intact() and S.intact() and loss.intact()
    return terms, S, loss


def run_bwd(dev, S, s_buf, up, B, N, Ds, cross, layout):
    d = Out(dev, B * N, 3 * Ds, BF16, ld=3 * Ds + 8)
    call("devit_qkv_pair_bwd", S.t, s_buf, torch.tensor(up, dtype=F32, device=dev), B, N, Ds, s_buf.stride(0), 64, cross, LAYOUT[layout], d.t, d.ld)
    assert d.intact(), "a write behind row B N of d or into its pad columns"
    assert not bool(torch.isnan(d.v).any()), "a live gradient element was not written"
    return d


# ============================================================================================ the kernels, per element
@pytest.mark.parametrize("regime", QM.REGIMES)
@pytest.mark.parametrize("B,N,Ds,Dt", QM.CASES)
def test_qkv_pair_kernels(dev, B, N, Ds, Dt, regime):
    """Both modes, both layouts: the loss, every ordered pair's row terms, every S slot and the gradient inside their per-element bounds around the
    float64 restatement; S zero outside N x N and in its K tail; guards behind terms, S, the loss and d (rows >= B N, pad columns) intact; every live
    gradient element written.  For the cross mode under the view map also: two runs give the same bits, and NaN or 1e30 in the rows behind B N and
    behind an image change no bit."""
    if regime == "same":
        Dt = Ds
    xs_c, xt_c, up = QM.inputs(B, N, Ds, Dt, regime)
    xs, xt = xs_c.to(dev), xt_c.to(dev)
    tdt = F16 if regime == "f16" else BF16
    s_buf, t_buf = packed(xs_c, BF16, dev, pad=8)[:, : 3 * Ds], packed(xt_c, tdt, dev)
    for cross, layout in MODES:
        tag = f"B{B}_N{N}_{Ds}_{Dt}/{regime}/{'cross' if cross else 'self'}/{layout}"
        r, bnd = QM.bounds(xs, xt, bool(cross), layout, layers=1, upstream=up)
        r1, bnd1 = QM.bounds(xs, xt, bool(cross), layout, layers=1, upstream=1.0)       # (the forward's S carries no upstream)
        terms, S, loss = run_fwd(dev, s_buf, t_buf, B, N, Ds, Dt, cross, layout)
        hold(f"{tag}/loss", loss.t[0, 0], r["loss"], bnd["loss"])
        Sv = S.t.view(-1, B, 208, 224)
        for (i, j), ref in r1["S"].items():
            slot = 3 * i + j if cross else i
            hold(f"{tag}/terms{i}{j}", terms.v[slot].view(B, N), r["terms"][(i, j)], bnd["terms"][(i, j)])
            hold(f"{tag}/S{i}{j}", Sv[slot, :, :N, :N], ref, bnd1["S"][(i, j)])
        assert not bool(Sv[:, :, N:].any()) and not bool(Sv[:, :, :, N:].any()), "S must be zero outside N x N"
        d = run_bwd(dev, S, s_buf, up, B, N, Ds, cross, layout)
        hold(f"{tag}/d", d.v.view(B, N, 3 * Ds), r["d"], bnd["d"])
        if regime == "same":
            # student == teacher: the gradient lies inside its bound around 0 (held above), the loss is the mean entropy of the softmaxes
            g = r["grams"]
            ent = sum((-(v["Ptr"] * torch.log(v["Ptr"])).sum(2)).sum() + ((-(v["Ptc"] * torch.log(v["Ptc"])).sum(1)).sum() if i != j else 0.)
                      for (i, j), v in g.items()) / (r["P"] * B * N)
            assert abs(float(ent) - float(r["loss"])) <= 1e-12 * max(1.0, float(ent))
        if cross and layout == "view":
            t2, S2, l2 = run_fwd(dev, s_buf, t_buf, B, N, Ds, Dt, cross, layout)
            d2 = run_bwd(dev, S2, s_buf, up, B, N, Ds, cross, layout)
            assert torch.equal(t2.flat, terms.flat) and torch.equal(S2.flat, S.flat) and torch.equal(l2.flat, loss.flat) and torch.equal(d2.flat, d.flat)
            for poison in (float("nan"), 1e30):
                sp, tp = packed(xs_c, BF16, dev, behind=poison), packed(xt_c, tdt, dev, behind=poison if tdt == BF16 else 6e4)
                t3, S3, l3 = run_fwd(dev, sp, tp, B, N, Ds, Dt, cross, layout)
                d3 = run_bwd(dev, S3, sp, up, B, N, Ds, cross, layout)
                assert torch.equal(t3.v, terms.v) and torch.equal(S3.t, S.t) and torch.equal(l3.t, loss.t) and torch.equal(d3.v, d.v), poison
                if B > 1:
                    # image 0 alone: what lies behind it -- the next image's rows, or poison -- is never read
                    one_s, one_t = packed(xs_c[:1], BF16, dev, behind=poison), packed(xt_c[:1], tdt, dev, behind=poison if tdt == BF16 else 6e4)
                    ta, Sa, la = run_fwd(dev, s_buf, t_buf, 1, N, Ds, Dt, cross, layout)
                    tb, Sb, lb = run_fwd(dev, one_s, one_t, 1, N, Ds, Dt, cross, layout)
                    da, db = run_bwd(dev, Sa, s_buf, up, 1, N, Ds, cross, layout), run_bwd(dev, Sb, one_s, up, 1, N, Ds, cross, layout)
                    assert torch.equal(ta.v, tb.v) and torch.equal(Sa.t, Sb.t) and torch.equal(la.t, lb.t) and torch.equal(da.v, db.v), poison


# ============================================================================================ the public functions
def as_views(buf, B, N, H, grad=False):
    """(q, k, v) [B, H, N, 64] views of a packed buffer, tagged as the models tag theirs"""
    D = H * 64
    buf = buf.requires_grad_(True) if grad else buf
    out = []
    for i in range(3):
        v = buf[: B * N, i * D:(i + 1) * D].view(B, N, H, 64).permute(0, 2, 1, 3)
        v._devit_packed = (buf, B, N, H)
        out.append(v)
    return tuple(out), buf


@pytest.mark.parametrize("cross", [0, 1])
def test_public_functions_packed_and_generic(dev, cross):
    """losses.cal_qkv_loss / cal_qkv_loss2 on the models' packed views give the bits of the kernels; generic [B, H, N, 64] tensors (a differentiable
    repack) give the bits of the packed path; a two-pair list gives the mean of its pairs and halves their gradients; an fp32 teacher buffer is cast
    to bf16; with D = 64 (one head) `view` and `tokens` give the same bits."""
    from devit_amd import losses
    fn = losses.cal_qkv_loss2 if cross else losses.cal_qkv_loss
    B, N, Ds, Dt = 2, 17, 128, 256
    pairs = []
    for li in range(2):
        xs_c, xt_c, _ = QM.inputs(B, N, Ds, Dt, "sharp" if li == 0 else "flat")
        pairs.append((xs_c, xt_c))
    singles = []
    for layout in ("view", "tokens"):
        for xs_c, xt_c in pairs:
            s_buf, t_buf = packed(xs_c, BF16, dev, extra=256), packed(xt_c, BF16, dev, extra=256)
            _, S, loss = run_fwd(dev, s_buf, t_buf, B, N, Ds, Dt, cross, layout)
            d = run_bwd(dev, S, s_buf, 1.0, B, N, Ds, cross, layout)
            sv, sb = as_views(s_buf.clone(), B, N, Ds // 64, grad=True)
            tv, _ = as_views(t_buf, B, N, Dt // 64)
            lp = fn([sv], [tv], layout=layout)
            lp.backward()
            assert torch.equal(lp.detach(), loss.t[0, 0]) and torch.equal(sb.grad[: B * N], d.v), layout
            # generic tensors: fp32 copies of the same values, no tag
            sg = [v.detach().float().clone().requires_grad_(True) for v in sv]
            lg = fn([tuple(sg)], [tuple(v.float().clone() for v in tv)], layout=layout)
            lg.backward()
            assert torch.equal(lg.detach(), lp.detach())
            for i, g in enumerate(sg):
                assert g.grad.dtype == F32 and torch.equal(g.grad, sb.grad[: B * N, i * Ds:(i + 1) * Ds].view(B, N, -1, 64).permute(0, 2, 1, 3).float())
            # an fp32 teacher buffer (the exact-fp32 teacher under a 16-bit student)
            tv32, _ = as_views(t_buf.float(), B, N, Dt // 64)
            assert torch.equal(fn([sv], [tv32], layout=layout).detach(), lp.detach())
            if layout == "view":
                singles.append((sv, tv, lp.detach(), sb.grad.clone()))
    # the two-pair list
    fresh = [as_views(s[0][0]._devit_packed[0].detach().clone(), B, N, Ds // 64, grad=True) for s in singles]
    both = fn([f[0] for f in fresh], [s[1] for s in singles])
    both.backward()
    mean = (singles[0][2].double() + singles[1][2].double()) / 2
    assert abs(float(both.detach()) - float(mean)) <= 2.0 ** -23 * float(mean)          # (each pair's kernel divides by 2; one fp32 addition)
    for (_, buf), s in zip(fresh, singles):
        lone = s[3][: B * N].double() / 2
        # d = bf16(up S X) with S rounded from a coefficient half as large: the halved S is the same bits (a power of two), so is d
        assert torch.equal(buf.grad[: B * N].double(), lone)
    # one head: the layouts coincide
    xs_c, xt_c, _ = QM.inputs(2, 16, 64, 64, "sharp")
    s_buf, t_buf = packed(xs_c, BF16, dev), packed(xt_c, BF16, dev)
    outs = []
    for layout in ("view", "tokens"):
        terms, S, loss = run_fwd(dev, s_buf, t_buf, 2, 16, 64, 64, cross, layout)
        outs.append((terms.flat, S.flat, loss.flat, run_bwd(dev, S, s_buf, 1.0, 2, 16, 64, cross, layout).flat))
    assert all(torch.equal(a, b) for a, b in zip(*outs))


def test_refusals(dev):
    """every refusal returns its exact code and writes nothing"""
    from devit_amd import _lib as L
    from devit_amd import losses
    lib = L.load()
    B, N, D = 1, 5, 128
    s = torch.zeros(64, 3 * D, dtype=BF16, device=dev)
    terms, S, loss, d = Out(dev, 9, B * N), Out(dev, 9 * B * 208, 224, BF16), Out(dev, 1, 1), Out(dev, B * N, 3 * D, BF16)
    up = torch.ones(1, device=dev)
    st = L.stream_ptr()

    def fwd(s_=s, t_=s, N_=N, Ds=D, Dt=D, ld=3 * D, hd_s=64, hd_t=64, cross=1, layout=0, layers=1, terms_=terms.t, S_=S.t, loss_=loss.t):
        return lib.devit_qkv_pair_fwd(L.ptr(s_), L.ptr(t_), B, N_, Ds, Dt, ld, ld, hd_s, hd_t, 0, cross, layout, layers, L.ptr(terms_), L.ptr(S_),
                                      L.ptr(loss_), st)

    def bwd(S_=S.t, s_=s, up_=up, N_=N, Ds=D, ld=3 * D, hd=64, cross=1, layout=0, d_=d.t, ld_d=3 * D):
        return lib.devit_qkv_pair_bwd(L.ptr(S_), L.ptr(s_), L.ptr(up_), B, N_, Ds, ld, hd, cross, layout, L.ptr(d_), ld_d, st)
    SHAPE, ARG = -1, -2
    assert fwd(N_=209) == SHAPE and bwd(N_=209) == SHAPE                              # N > 208
    assert fwd(hd_s=32) == SHAPE and fwd(hd_t=32) == SHAPE and bwd(hd=32) == SHAPE    # head width 32
    assert fwd(Ds=96, ld=384) == SHAPE and fwd(Dt=96, ld=384) == SHAPE and bwd(Ds=96) == SHAPE      # width 96
    assert fwd(Ds=1088, ld=3264) == SHAPE and fwd(ld=3 * D - 8) == SHAPE and fwd(ld=3 * D + 4) == SHAPE and bwd(ld_d=3 * D - 4) == SHAPE
    assert fwd(s_=None) == ARG and fwd(t_=None) == ARG and fwd(terms_=None) == ARG and fwd(S_=None) == ARG and fwd(loss_=None) == ARG
    assert bwd(S_=None) == ARG and bwd(s_=None) == ARG and bwd(up_=None) == ARG and bwd(d_=None) == ARG
    assert fwd(cross=2) == ARG and fwd(cross=-1) == ARG and fwd(layout=2) == ARG and fwd(layers=0) == ARG and bwd(cross=2) == ARG and bwd(layout=-1) == ARG
    assert fwd(s_=s.view(-1)[4:]) == ARG and bwd(d_=d.flat[1:]) == ARG                # misaligned
    x = torch.zeros(4, 7, device=dev)
    assert lib.devit_soft_ce_rows_fwd(L.ptr(x), L.ptr(x), 0, 7, L.ptr(terms.t), L.ptr(loss.t), st) == SHAPE
    assert lib.devit_soft_ce_rows_fwd(L.ptr(x), L.ptr(x), 4, 0, L.ptr(terms.t), L.ptr(loss.t), st) == SHAPE
    assert lib.devit_soft_ce_rows_fwd(None, L.ptr(x), 4, 7, L.ptr(terms.t), L.ptr(loss.t), st) == ARG
    assert lib.devit_soft_ce_rows_bwd(L.ptr(x), L.ptr(x), None, 4, 7, L.ptr(terms.t), st) == ARG
    assert lib.devit_soft_ce_rows_bwd(L.ptr(x), L.ptr(x), L.ptr(up), 4, -1, L.ptr(terms.t), st) == SHAPE
    torch.cuda.synchronize()
    for o in (terms, S, loss, d):
        assert o.intact() and bool(torch.isnan(o.v.float()).all()), "a refused call wrote"
    # the public functions
    q32 = torch.zeros(1, 4, 5, 32, device=dev)
    q = torch.zeros(1, 2, 5, 64, device=dev)
    with pytest.raises(L.DevitError):
        losses.cal_qkv_loss([(q32, q32, q32)], [(q, q, q)])                           # head width 32
    with pytest.raises(L.DevitError):
        losses.cal_qkv_loss2([(q, q, q)], [(q[:, :, :4], q[:, :, :4], q[:, :, :4])])  # token counts differ
    with pytest.raises(L.DevitError):
        big = torch.zeros(1, 1, 209, 64, device=dev)
        losses.cal_qkv_loss([(big, big, big)], [(big, big, big)])                     # N > 208
    with pytest.raises(ValueError):
        losses.cal_qkv_loss([(q, q, q)], [(q, q, q)], layout="heads")
    sv, _ = as_views(torch.zeros(64, 384, dtype=F32, device=dev), 1, 5, 2)               # a precision="f32" student's packed buffer
    tv, _ = as_views(torch.zeros(64, 384, dtype=BF16, device=dev), 1, 5, 2)
    for fn in (losses.cal_qkv_loss, losses.cal_qkv_loss2):
        with pytest.raises(NotImplementedError, match="f32"):
            fn([sv], [tv])


@pytest.mark.parametrize("shape", [(5, 7), (64, 198), (3, 1), (2, 5, 5)])
def test_soft_cross_entropy(dev, shape):
    """soft_cross_entropy against float64 inside the bounds of _qkvce_model.soft_ce_bounds: C below, at and above a wave's 64 lanes, C = 1 (loss 0,
    gradient 0), more rows than one block's four, a 3-D input; guards intact; a negative upstream"""
    from devit_amd import losses
    p_c = torch.from_numpy(QM.det_array(f"qkvce/sce/p{shape}", shape, std=3.0))
    t_c = torch.from_numpy(QM.det_array(f"qkvce/sce/t{shape}", shape, std=3.0))
    loss64, dp64, e_loss, e_dp = QM.soft_ce_bounds(p_c, t_c, upstream=-0.75)
    R, C = p_c.numel() // shape[-1], shape[-1]
    p, t = p_c.to(dev), t_c.to(dev)
    row_loss, loss, dp = Out(dev, 1, R), Out(dev, 1, 1), Out(dev, R, C)
    call("devit_soft_ce_rows_fwd", p, t, R, C, row_loss.t, loss.t)
    call("devit_soft_ce_rows_bwd", p, t, torch.tensor(-0.75, device=dev), R, C, dp.t)
    assert row_loss.intact() and loss.intact() and dp.intact()
    hold(f"sce/{shape}/loss", loss.t[0, 0], loss64, e_loss)
    hold(f"sce/{shape}/dp", dp.v.view(shape), dp64, e_dp)
    pg = p.clone().requires_grad_(True)
    lp = losses.soft_cross_entropy(pg, t)
    (lp * -0.75).backward()
    assert torch.equal(lp.detach(), loss.t[0, 0]) and torch.equal(pg.grad, dp.v.view(shape))
    if C == 1:
        assert float(lp.detach()) == 0.0 and float(pg.grad.abs().max()) == 0.0


# ============================================================================================ the step
# |k_loss - oracle| / oracle of the UNMODIFIED step, `dedeit` under DeiT-B, B = 4, S = 112, on seven seeded batches on the MI355X
# (profiles/qkvce_parity_margins.json; `deviations` below measures one): the yardstick of the two new losses' parity with the CPU oracle
K_LOSS_DEVIATIONS = (3.29e-05, 3.89e-04, 2.12e-04, 9.67e-05, 1.27e-04, 1.11e-04, 2.77e-04)
QKV_LOSS_BAR = 2 * max(K_LOSS_DEVIATIONS)       # 7.78e-4


def oracle_step(st_s, st_t, img, soft, dps):
    """the CPU oracle's forward step (fp32) + the float64 definitions of the two new losses on its middle blocks' q/k/v"""
    with torch.no_grad():
        ref = IM.distill_step(st_s, GS, st_t, GT, img, soft, dp_scales=dps)
    s_qkv = tuple(x.to(F64) for x in ref["student"]["qkv"][GS["depth"] // 2 - 1])
    t_qkv = tuple(x.to(F64) for x in ref["teacher"]["qkv"][GT["depth"] // 2 - 1])
    ref["qkv_ce_loss"] = QM.reference_form([s_qkv], [t_qkv], False)
    ref["qkv_cross_loss"] = QM.reference_form([s_qkv], [t_qkv], True)
    return ref


def engine_step(dev, s, t, img, soft, dps, **kw):
    from devit_amd import engine
    s.train()
    for p in s.parameters():
        p.grad = None
    return engine.distill_forward(s, t, img.to(dev), soft.to(dev), gama=(0.2, 0.1, 0.3), kind="hard", alpha=0.5, tau=1.0,
                                  dp_scales=[(a.to(dev).contiguous(), b.to(dev).contiguous()) for a, b in dps], **kw)


def deviations(dev, seed):
    """(k_loss, qkv_ce_loss, qkv_cross_loss) relative deviations from the CPU oracle of one seeded batch"""
    s, st_s, t, st_t, img, soft, dps = step_setup(dev, 112, tag=f"qkvce/step{seed}")
    ref = oracle_step(st_s, st_t, img, soft, dps)
    with torch.no_grad():
        out = engine_step(dev, s, t, img, soft, dps, qkv_ce_gama=0.5, qkv_cross_gama=0.25)
    return {k: abs(float(out[k]) - float(ref[k])) / abs(float(ref[k])) for k in ("k_loss", "qkv_ce_loss", "qkv_cross_loss")}


@pytest.fixture(scope="module")
def qkv_step(dev):
    return step_setup(dev, 112, tag="qkvce/step0")


def test_step_with_qkv_weights(dev, monkeypatch, qkv_step):
    """distill_forward(qkv_ce_gama=0.5, qkv_cross_gama=0.25), `dedeit` under DeiT-B, B = 4, S = 112, fixed DropPath scales.
    (i) the two new losses and their gradients into the student's packed qkv buffer, against the float64 restatement evaluated on the step's OWN
        bf16 qkv buffers: inside the derived bounds.
    (ii) each new loss against the CPU oracle's fp32 step + the float64 definitions on the oracle's q/k/v.  The bar is not fixed in advance: it is
        2 x the worst relative deviation of the unmodified k_loss from the oracle over seven seeded batches (K_LOSS_DEVIATIONS above):
        k_loss        3.29e-05, 3.89e-04, 2.12e-04, 9.67e-05, 1.27e-04, 1.11e-04, 2.77e-04   -> bar 2 x 3.89e-4 = 7.78e-4
        qkv_ce_loss   8.40e-05, 1.07e-04, 4.90e-04, 2.32e-04, 1.33e-04, 3.48e-04, 1.76e-04   (worst 4.90e-4)
        qkv_cross_loss 1.68e-05, 6.52e-07, 4.84e-06, 6.04e-06, 7.95e-06, 2.58e-06, 1.06e-05  (worst 1.68e-5)
        on the MI355X; this test's batch is the first of the seven."""
    from devit_amd import losses
    s, st_s, t, st_t, img, soft, dps = qkv_step
    seen = {}
    for name in ("cal_qkv_loss", "cal_qkv_loss2"):
        orig = getattr(losses, name)

        def spy(stu, tea, layout="view", _orig=orig, _name=name):
            seen[_name] = (stu[0], tea[0])
            return _orig(stu, tea, layout=layout)
        monkeypatch.setattr(losses, name, spy)
    out = engine_step(dev, s, t, img, soft, dps, qkv_ce_gama=0.5, qkv_cross_gama=0.25)
    assert set(out) == {"loss", "cls_loss", "q_loss", "k_loss", "v_loss", "logits", "teacher_logits", "qkv_ce_loss", "qkv_cross_loss"}
    (s_buf, B, N, Hs), (t_buf, _, _, Ht) = seen["cal_qkv_loss"][0][0]._devit_packed, seen["cal_qkv_loss"][1][0]._devit_packed
    assert seen["cal_qkv_loss2"][0][0]._devit_packed[0] is s_buf and s_buf.dtype == BF16 and (B, N) == (4, 51)
    xs = s_buf.detach()[: B * N].to(F64).view(B, N, -1)
    xt = t_buf.detach()[: B * N].to(F64).view(B, N, -1)
    for key, cross in (("qkv_ce_loss", False), ("qkv_cross_loss", True)):
        r, bnd = QM.bounds(xs, xt, cross, "view", layers=1, upstream=1.0)
        hold(f"step/{key}", out[key].detach(), r["loss"], bnd["loss"])
        d, = torch.autograd.grad(out[key], s_buf, retain_graph=True)
        hold(f"step/{key}/d", d[: B * N].view(B, N, -1), r["d"], bnd["d"])
    total = out["cls_loss"].double() + 0.2 * out["q_loss"].double() + 0.1 * out["k_loss"].double() + 0.3 * out["v_loss"].double() \
        + 0.5 * out["qkv_ce_loss"].double() + 0.25 * out["qkv_cross_loss"].double()
    assert abs(float(out["loss"].detach()) - float(total.detach())) <= 4 * 2.0 ** -23 * abs(float(total.detach()))
    # the whole backward, on a step of its own (the nodes above gave their S away to the two gradient calls)
    engine_step(dev, s, t, img, soft, dps, qkv_ce_gama=0.5, qkv_cross_gama=0.25)["loss"].backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in s.parameters() if p.requires_grad)
    ref = oracle_step(st_s, st_t, img, soft, dps)
    fails = []
    for key in ("k_loss", "qkv_ce_loss", "qkv_cross_loss"):
        e = abs(float(out[key].detach()) - float(ref[key])) / abs(float(ref[key]))
        print(f"qkvce step {key}: {float(out[key].detach()):.6f} vs {float(ref[key]):.6f} rel {e:.3e}")
        if key != "k_loss" and not chk(e, QKV_LOSS_BAR, name=f"qkvce/step/{key}"):
            fails.append((key, e))
    assert not fails, fails
    for p in s.parameters():
        p.grad = None


def test_zero_weights_are_the_step_as_it_was(dev, monkeypatch, qkv_step):
    """both weights 0: the returned keys, the losses and every gradient are the bits of the call without the arguments"""
    one_k_slice(monkeypatch)
    s, _, t, _, img, soft, dps = qkv_step

    def run(**kw):
        out = engine_step(dev, s, t, img, soft, dps, **kw)
        out["loss"].backward()
        torch.cuda.synchronize()
        return out, {n: p.grad.detach().clone() for n, p in s.named_parameters()}
    o0, g0 = run()
    o1, g1 = run(qkv_ce_gama=0.0, qkv_cross_gama=0.0, qkv_layout="tokens")
    assert set(o0) == set(o1) == {"loss", "cls_loss", "q_loss", "k_loss", "v_loss", "logits", "teacher_logits"}
    for k in ("loss", "cls_loss", "q_loss", "k_loss", "v_loss"):
        assert torch.equal(o0[k], o1[k]), k
    diff = [n for n in g0 if not torch.equal(g0[n], g1[n])]
    assert not diff, diff
    for p in s.parameters():
        p.grad = None


# ============================================================================================ the CLI
def test_distill_sub_qkv_cli(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import distill_sub
    parser = argparse.ArgumentParser(parents=[distill_sub.get_args_parser()])
    args = parser.parse_args(["--synthetic", "2", "--batch-size", "8", "--input-size", "32", "--epochs", "1", "--qkv-ce-gama", "0.3",
                              "--qkv-cross-gama", "0.1", "--model", "dedeit", "--teacher-model", "deit_base_distilled_patch16_224",
                              "--dataset", "cifar100", "--num_division", "4", "--output_dir", str(tmp_path), "--warmup-epochs", "0"])
    distill_sub.main(args)
    line = json.loads(open(os.path.join(args.output_dir, "sub-dataset0", "log.txt")).read().splitlines()[-1])
    for k in ("train_qkv_ce_loss", "train_qkv_cross_loss", "train_loss"):
        assert np.isfinite(line[k]) and line[k] > 0, (k, line[k])
