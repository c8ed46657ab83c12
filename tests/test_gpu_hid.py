"""Hidden-state distillation on a real MI355X: the csrc/hid.hip kernels and the Gram / gradient GEMMs between them held per element to the float64
model of tests/_hid_model.py; the injection kernel bit for bit; gradients into the exposed 'encoder' outputs of the 16-bit path against the same
model on precision="f32" (an already-supported path: the yardstick, not the code under test); the DEKD step with --hid-gama against the CPU oracle;
the CLI.  Every figure goes through conftest.chk into the session's parity_margins.json."""
import argparse
import json
import os

import numpy as np
import pytest
import torch

import _hid_model as HM
import _imgsize_model as IM
from conftest import chk
from oracle import devit_oracle as O
from oracle.detgen import det_array, det_labels
from test_gpu_imgsize import SLICES, model_at, rel
from test_gpu_tail import Out, call, same_bits

pytestmark = pytest.mark.gpu
F32, BF16 = torch.float32, torch.bfloat16
C = 25
GS, GT = O.GEOMETRY["dedeit"], O.GEOMETRY["deit_base_distilled_patch16_224"]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from devit_amd import _lib
    _lib.require_device(torch.zeros(1, device="cuda"))
    return torch.device("cuda")


def hold(tag, got, ref, bnd):
    r = HM.ratio(got, ref, bnd)
    print(f"hid/{tag} {r:.3f}")
    assert chk(r, 1.0, name=f"hid/{tag}"), f"hid/{tag}: worst |err| / bound {r:.3f}"


# ============================================================================================ the loss kernels, per element
@pytest.mark.parametrize("regime", HM.REGIMES)
@pytest.mark.parametrize("B,N,Ds,Dt", HM.CASES)
def test_hid_kernels(dev, B, N, Ds, Dt, regime):
    """h^, the inverse norms, the loss, S and dh of one (student, teacher) pair, each inside its per-element bound; zeros where zeros are promised;
    nothing written outside the outputs; the public cal_hid_relation_loss gives the same bits."""
    from devit_amd import losses, ops
    if regime == "same":
        Dt = Ds
    s_c, t_c = HM.inputs(B, N, Ds, Dt, regime)
    up = 0.5
    r, bnd = HM.bounds(s_c, t_c, layers=1, upstream=up)
    s, t = s_c.to(dev), t_c.to(dev)
    M, tag = B * N, f"B{B}_N{N}_{Ds}_{Dt}/{regime}"
    hs, inv_s = ops.hid_normalize(s)
    ht, _ = ops.hid_normalize(t)
    ld = hs.shape[1]
    assert hs.dtype == BF16 and ld % 128 == 0 and hs.shape[0] >= (B - 1) * N + 256
    hold(f"{tag}/hn", hs[:M, :Ds].view(B, N, Ds), r["hs"], bnd["hs"])
    hold(f"{tag}/inv", inv_s.view(B, N), r["inv_s"], bnd["inv_s"])
    assert not bool(hs[M:].any()) and not bool(hs[:, Ds:].any()) and not bool(ht[M:].any()), "overhang rows / pad columns of h^ must be zero"
    gs, gt = ops.hid_gram(hs, B, N, Ds), ops.hid_gram(ht, B, N, Dt)
    loss = ops.hid_stats(gs, gt, B, N, 1)
    hold(f"{tag}/loss", loss[0], r["loss"], bnd["loss"])
    upstream = torch.tensor(up, dtype=F32, device=dev)
    S = Out(dev, B * 256, 256, BF16)
    call("devit_hid_grad", gs, gt, upstream, B, N, 256, 1, S.t, 0)
    assert S.intact()
    Sv = S.t.view(B, 256, 256)
    hold(f"{tag}/S", Sv[:, :N, :N], r["S"], bnd["S"])
    assert not bool(Sv[:, N:].any()) and not bool(Sv[:, :, N:].any()), "S must be zero outside N x N"
    dhn = ops.hid_dhn(Sv, hs, B, N, Ds)
    dh = Out(dev, M, Ds)
    call("devit_hid_normalize_bwd", hs, dhn, inv_s, dh.t, B, N, Ds, ld, 0)
    assert dh.intact(), "a write behind row B N of dh"
    hold(f"{tag}/dh", dh.v.view(B, N, Ds), r["dh"], bnd["dh"])
    # the public entry: the same kernels behind autograd
    sg = s.clone().requires_grad_(True)
    lp = losses.cal_hid_relation_loss([sg], [t])
    (lp * up).backward()
    assert torch.equal(lp.detach(), loss[0]) and torch.equal(sg.grad.view(M, Ds), dh.v)
    assert bool(torch.isfinite(sg.grad).all()) and bool(torch.isfinite(lp))
    if regime == "same":
        assert float(lp.detach()) == 0.0 and float(sg.grad.abs().max()) == 0.0
    if regime == "zero_row":
        assert float(hs[N // 2, :Ds].abs().max()) == 0.0 and float(inv_s[N // 2]) == pytest.approx(1e12, rel=1e-6)


def test_hid_list_form_and_exact_mode(dev, golden):
    """two layer pairs of different content: the list form divides by the number of pairs (the reference's golden values); exact=True (fp32 h^,
    devit_gemm_f32) meets the f32 bars: loss 1e-4, gradient 1e-3 of its maximum"""
    from devit_amd import losses
    g = golden("hid_relation")
    stu, tea = HM.golden_inputs()
    for exact, lbar, gbar in ((True, 1e-4, 1e-3), (False, 5e-4, 1.5e-2)):
        ss = [x.to(dev).requires_grad_(True) for x in stu]
        loss = losses.cal_hid_relation_loss(ss, [x.to(dev) for x in tea], exact=exact)
        loss.backward()
        e = abs(float(loss.detach()) - float(g["loss"])) / abs(float(g["loss"]))
        print(f"hid golden exact={exact} loss rel {e:.3e}")
        assert chk(e, lbar, name=f"hid/golden/exact{int(exact)}/loss")
        for i, x in enumerate(ss):
            e = rel(x.grad, g[f"grad_s{i}"])
            print(f"hid golden exact={exact} grad {i} rel {e:.3e}")
            assert chk(e, gbar, name=f"hid/golden/exact{int(exact)}/grad{i}")


def test_hid_refusals(dev):
    from devit_amd import _lib as L
    from devit_amd import losses
    with pytest.raises(L.DevitError):
        losses.cal_hid_relation_loss([torch.zeros(1, 209, 64, device=dev)], [torch.zeros(1, 209, 64, device=dev)])      # N > 208
    with pytest.raises(L.DevitError):
        losses.cal_hid_relation_loss([torch.zeros(1, 4, 96, device=dev)], [torch.zeros(1, 4, 64, device=dev)])          # D % 64
    with pytest.raises(L.DevitError):
        losses.cal_hid_relation_loss([torch.zeros(2, 4, 64, device=dev)], [torch.zeros(2, 5, 64, device=dev)])          # token counts differ
    with pytest.raises(L.DevitError):
        losses.cal_hid_relation_loss([torch.zeros(2, 4, 64)], [torch.zeros(2, 4, 64)])                                  # no CPU fallback
    x = torch.zeros(8, 64, device=dev)
    lib = L.load()
    assert lib.devit_hid_stats(L.ptr(x), L.ptr(x), 1, 4, 128, 1, L.ptr(x), L.ptr(x), L.stream_ptr()) == -1              # ldr != 256: DEVIT_ERR_SHAPE
    assert lib.devit_hid_normalize(L.ptr(x), L.ptr(x), L.ptr(x), 1, 4, 64, 64, 8, 0, 1e-12, L.stream_ptr()) == -1       # ld % 128
    assert lib.devit_add_scale_cast_bf16(L.ptr(x), L.ptr(x), L.ptr(x), None, 0, 8, 62, L.stream_ptr()) == -1            # D % 4


# ============================================================================================ the injection kernel, bit for bit
@pytest.mark.parametrize("M,D,rps", HM.inject_cases())
def test_add_scale_cast_bit_for_bit(dev, M, D, rps):
    dx_c = torch.from_numpy(det_array(f"hid/inj/dx{M}x{D}", (M, D)))
    add_c = torch.from_numpy(det_array(f"hid/inj/add{M}x{D}", (M, D), std=0.3))
    dx, add = dx_c.to(dev), add_c.to(dev)
    scale = None
    if rps:
        scale = torch.tensor([0.0 if b % 3 == 2 else 1.0 / 0.9 for b in range(M // rps + 1)], dtype=F32, device=dev)
    g = Out(dev, M, D, BF16)
    before = add.clone()
    call("devit_add_scale_cast_bf16", dx, add, g.t, scale, rps, M, D)
    want = dx_c.to(dev) + add
    assert torch.equal(dx, want), "dx + add must be torch's fp32 add"
    rows = torch.arange(M, device=dev) // rps if rps else None
    want_g = (want * scale[rows][:, None] if rps else want).to(BF16)
    assert same_bits(g.v, want_g) and g.intact() and torch.equal(add, before)


# ============================================================================================ gradients into the 'encoder' outputs
_enc_models = {}


def enc_model(dev, S, drop=0.0):
    import devit_amd
    key = (S, drop)
    if key not in _enc_models:
        torch.manual_seed(1234)
        m = devit_amd.create_model("dedeit", depth=3, num_classes=10, drop_path_rate=0.1, img_size=S, drop_rate=drop)
        with torch.no_grad():
            for n, p in m.named_parameters():          # biases and LayerNorm affines away from 0 / 1, as the oracle's weights
                if n.endswith("bias"):
                    p.normal_(0.0, 0.02)
        _enc_models[key] = m.to(dev).train()
    return _enc_models[key]


def enc_inputs(dev, S, B, seed=0):
    """(images, fixed DropPath scales with one dropped branch, one W per block)"""
    N = (S // 16) ** 2 + 2
    img = torch.from_numpy(det_array(f"hid/enc/img{S}/{seed}", (B, 3, S, S))).to(dev)
    g = torch.Generator().manual_seed(100 + seed)
    keep = 1.0 - torch.linspace(0, 0.1, 3)
    sc = torch.floor(keep.view(3, 1, 1) + torch.rand((3, 2, B), generator=g)) / keep.view(3, 1, 1)
    sc[2, 1, 0] = 0.0                                   # sample 0 drops block 2's MLP branch
    sc[1, 0, B - 1] = 0.0                               # the last sample drops block 1's attention branch
    dps = [(sc[i, 0].contiguous().to(dev), sc[i, 1].contiguous().to(dev)) for i in range(3)]
    Ws = [torch.from_numpy(det_array(f"hid/enc/W{i}/{S}/{seed}", (B, N, 384), std=0.05)).to(dev) for i in range(3)]
    return img, dps, Ws


def enc_run(vit, img, dps, Ws, sel=None, lean=False, seed=None, want_enc=True, top_direct=None):
    """sum(logits) + sum_i <enc_i, W_i> -> (loss, (logits, logits_dist), encs); top_direct: a W added on the encoder OUTPUT itself instead"""
    from devit_amd import de_vit
    x = vit.embed(img)
    xo, _, _, encs = de_vit.run_blocks(list(vit.blocks), x, True, False, False, want_enc, grad_ready=vit.grad_ready, dp_scales=dps,
                                       precision=vit.precision, enc_layers=sel, lean_tokens=vit.num_tokens if lean else 0, dropout_seed=seed)
    heads = vit._tokens_and_logits(xo, True)
    loss = heads[1].sum() + heads[2].sum()
    if top_direct is not None:
        loss = loss + (xo * top_direct).sum()
    for e, W in zip(encs or (), Ws):
        if e is not None and W is not None:
            loss = loss + (e * W).sum()
    return loss, (heads[1], heads[2]), encs


def grads_of(vit, loss):
    for p in vit.parameters():
        p.grad = None
    loss.backward()
    torch.cuda.synchronize()
    out = {n: p.grad.detach().clone() for n, p in vit.named_parameters()}
    for p in vit.parameters():
        p.grad = None
    return out


def deviation(got, ref):
    """(worst gradient-norm deviation, relative with the project's floor; worst |difference| of a parameter's gradient over its largest element)"""
    names = list(ref)
    gn = np.array([float(got[n].float().norm()) for n in names])
    rn = np.array([float(ref[n].float().norm()) for n in names])
    norms = float((np.abs(gn - rn) / (rn + 1e-3 * rn.max())).max())
    return norms, max(rel(got[n], ref[n]) for n in names)


# The project's bf16 bars (test_gpu_model.py::test_distill_step_vs_golden): gradient norms 3e-3, gradients 1.5e-2 of their maximum.  Measured on the
# MI355X, bf16 against precision="f32", seven seeded batches per shape, worst: this three-block model with the gradient entering
# only at the top (the path that existed) norms 1.3e-3, gradients 1.14e-2; with a gradient at every block norms 1.1e-3, gradients 1.03e-2 -- both
# bars stay.  With dropout 0.1 the same model measures 1.39e-2 already with the gradient at the top only and 1.45e-2 with all of them (norms
# 1.4e-3): that one bar moves to 2 x the worst of the seven, 2.9e-2.
ENC_NORM_BAR, ENC_GRAD_BAR, ENC_GRAD_BAR_DROPOUT = 3e-3, 1.5e-2, 2.9e-2

ENC_CASES = [("base", 32, 3, {}), ("base", 224, 2, {}), ("block_policy", 224, 2, {"DEVIT_WGRAD_GROUP": "block"}),
             ("block_policy", 32, 3, {"DEVIT_WGRAD_GROUP": "block"}), ("no_wgrad_stream", 224, 2, {"DEVIT_WGRAD_STREAM": "0"}),
             ("all_policy", 224, 2, {"DEVIT_WGRAD_GROUP": "all"}), ("dropout", 224, 2, {}), ("lean_selector", 224, 2, {}),
             ("compacted", 224, 2, {})]


@pytest.mark.parametrize("variant,S,B,env", ENC_CASES)
def test_encoder_output_gradients(dev, monkeypatch, variant, S, B, env):
    """sum(logits) + sum_i <enc_i, W_i> on the bf16 path against the same weights, DropPath scales (and dropout masks) on precision="f32":
    every parameter's gradient norm and gradient."""
    from devit_amd import shrink
    vit = enc_model(dev, S, drop=0.1 if variant == "dropout" else 0.0)
    img, dps, Ws = enc_inputs(dev, S, B)
    seed = 4242 if variant == "dropout" else None
    sel, lean = (({0}, True) if variant == "lean_selector" else (None, False))
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    try:
        if variant == "compacted":
            g = torch.Generator().manual_seed(5)
            for blk in vit.blocks:
                hm, nm = torch.ones(6), torch.ones(1536)
                hm[torch.randperm(6, generator=g)[:2]] = 0
                nm[torch.randperm(1536, generator=g)[:461]] = 0
                blk.attn.gate, blk.mlp.gate = hm, nm
        vit.precision = "f32"
        loss_r, logits_r, encs_r = enc_run(vit, img, dps, Ws, sel=sel, seed=seed)
        ref = grads_of(vit, loss_r)
        vit.precision = "bf16"
        if variant == "compacted":
            shrink.compact(vit, trainable=True)
        loss, logits, encs = enc_run(vit, img, dps, Ws, sel=sel, lean=lean, seed=seed)
        if sel is not None:
            assert [e is not None for e in encs] == [i in sel for i in range(3)]
            assert vit.blocks[-1].attn.head_output is None, "the lean tail was not taken"
        for i, (e, er) in enumerate(zip(encs, encs_r)):
            if e is not None:
                assert chk(rel(e, er), 1.5e-2, name=f"hid/enc/{variant}/S{S}/enc{i}")
        got = grads_of(vit, loss)
        norms, worst = deviation(got, ref)
        print(f"hid enc {variant} S{S} B{B}: grad norms {norms:.3e}  gradients {worst:.3e}")
        ok_n = chk(norms, ENC_NORM_BAR, name=f"hid/enc/{variant}/S{S}/grad_norms")
        ok_g = chk(worst, ENC_GRAD_BAR_DROPOUT if variant == "dropout" else ENC_GRAD_BAR, name=f"hid/enc/{variant}/S{S}/gradients")
        assert ok_n and ok_g, (norms, worst)
    finally:
        vit.precision = "bf16"
        if variant == "compacted":
            shrink.uncompact(vit)
            for blk in vit.blocks:
                blk.attn.gate, blk.mlp.gate = torch.ones(6), torch.ones(1536)


def one_k_slice(monkeypatch):
    """Bit-for-bit comparisons of two backward passes need sums with ONE order.  The patch-embedding weight gradient is a split-K GEMM whose slices add
    their partial sums with fp32 atomics in arrival order (ops.split_k_for: up to 16 slices here): two runs of the SAME call differ in its last bits
    (measured on the MI355X, four runs, that parameter alone).  With one slice every element is one add into the zeroed gradient."""
    from devit_amd import ops
    monkeypatch.setattr(ops, "split_k_for", lambda out_rows, out_cols, ksteps: 1)


@pytest.mark.parametrize("S,B", [(32, 3), (224, 2)])
def test_top_block_gradient_is_the_output_gradient(dev, monkeypatch, S, B):
    """a gradient given only for the top block's exposed output = the same tensor added to the encoder output's gradient: bit-identical parameter
    gradients"""
    one_k_slice(monkeypatch)
    vit = enc_model(dev, S)
    img, dps, Ws = enc_inputs(dev, S, B)
    a = grads_of(vit, enc_run(vit, img, dps, [None, None, Ws[2]])[0])
    b = grads_of(vit, enc_run(vit, img, dps, Ws, want_enc=False, top_direct=Ws[2])[0])
    diff = [n for n in a if not torch.equal(a[n], b[n])]
    assert not diff, diff


@pytest.mark.parametrize("S,B", [(32, 3), (224, 2)])
def test_selector_keeps_the_lean_tail(dev, S, B):
    """enc_layers without the last block: its entry is None, the tail runs lean, and the logits are the bits of the run without a selector"""
    vit = enc_model(dev, S)
    img, dps, Ws = enc_inputs(dev, S, B)
    with torch.no_grad():
        _, plain, _ = enc_run(vit, img, dps, Ws, lean=True, want_enc=False)
        _, full, encs_all = enc_run(vit, img, dps, Ws, lean=True)                     # every layer handed out: the tail is not lean
        assert vit.blocks[-1].attn.head_output is not None and all(e is not None for e in encs_all)
        _, picked, encs = enc_run(vit, img, dps, Ws, sel={0, 1}, lean=True)
    assert encs[2] is None and encs[0] is not None and encs[1] is not None and vit.blocks[-1].attn.head_output is None
    assert torch.equal(picked[0], plain[0]) and torch.equal(picked[1], plain[1])
    assert torch.equal(full[0], plain[0]) and torch.equal(full[1], plain[1])
    assert torch.equal(encs[0], encs_all[0]) and torch.equal(encs[1], encs_all[1])


def test_attention_output_gradients_stay_refused(dev):
    from devit_amd import _lib as L
    vit = enc_model(dev, 32)
    img, _, _ = enc_inputs(dev, 32, 3)
    out = vit(img, output_att=True)
    with pytest.raises(L.DevitError, match="'attention' outputs"):
        out["attention"][1].float().sum().backward()
    for p in vit.parameters():
        p.grad = None


# ============================================================================================ the step
HID_LOSS_BAR = 1.75e-3       # 2 x 8.74e-4, the worst of seven seeded batches per size on the MI355X: see test_step_with_hid_gama's docstring


def step_setup(dev, S, B=4, tag="hid/step"):
    s, st_s = model_at("dedeit", S, dev, drop_path_rate=0.1)
    t, st_t = model_at("deit_base_distilled_patch16_224", S, dev)
    t.eval()
    for p in t.parameters():
        p.requires_grad_(False)
    img = torch.from_numpy(det_array(f"{tag}/img{S}", (B, 3, S, S)))
    y1, y2 = det_labels(f"{tag}/y1", B, C), det_labels(f"{tag}/y2", B, C)
    oh = lambda y: torch.full((B, C), 0.1 / C).scatter_(1, torch.from_numpy(y)[:, None], 1 - 0.1 + 0.1 / C)
    soft = oh(y1) * 0.7 + oh(y2) * 0.3
    dps = IM.dp_scales_for(f"{tag}/{S}", B)
    return s, st_s, t, st_t, img, soft, dps


def oracle_step(st_s, st_t, img, soft, dps, hid_gama, backward=True):
    """the CPU oracle's step + hid_gama * the definition of the hidden-state loss on its 'encoder' outputs (block i's output is entry i + 1)"""
    ref_st = {k: v.clone().requires_grad_(backward) for k, v in st_s.items()}
    ref = IM.distill_step(ref_st, GS, st_t, GT, img, soft, dp_scales=dps)
    s_h, t_h = ref["student"]["encoder"][GS["depth"] // 2], ref["teacher"]["encoder"][GT["depth"] // 2].detach()
    ref["hid_loss"] = HM.autograd_loss([s_h], [t_h])
    r64 = HM.restate(s_h.detach(), t_h)
    assert abs(float(r64["loss"]) - float(ref["hid_loss"].detach())) <= 1e-5 * float(r64["loss"])
    ref["loss"] = ref["loss"] + hid_gama * ref["hid_loss"]
    grads = None
    if backward:
        ref["loss"].backward()
        grads = {k: v.grad for k, v in ref_st.items()}
    return ref, grads


@pytest.fixture(scope="module", params=[112, 224])
def hid_step(dev, request):
    S = request.param
    s, st_s, t, st_t, img, soft, dps = step_setup(dev, S)
    ref, grads = oracle_step(st_s, st_t, img, soft, dps, 0.5)
    return S, s, t, img, soft, dps, ref, grads


@pytest.mark.parametrize("precision", ["bf16", "f32"])
def test_step_with_hid_gama(dev, hid_step, precision):
    """distill_forward(hid_gama=0.5), `dedeit` under DeiT-B, B = 4, fixed DropPath scales, against the CPU oracle: the six losses, every gradient norm
    and the gradient slices test_distill_step_vs_golden samples.  bf16 bars are the project's (losses 5e-4, norms 3e-3, slices 1.5e-2); precision="f32"
    (exact=True) meets the f32 bars (1e-4, 1e-3).  The bf16 hid_loss bar is a measurement, not the project's 5e-4: bf16 `dedeit` / DeiT-B against the CPU
    oracle's fp32 forward and the float64 restatement on seven seeded batches per size gave 4.4e-4 .. 8.7e-4 at S = 112 and 3.2e-4 .. 6.6e-4 at
    S = 224 on the MI355X (the hidden states themselves carry six bf16 blocks of rounding; the loss kernels alone on the oracle's hidden states:
    DESIGN.md section 13); HID_LOSS_BAR = 2 x the worst = 1.75e-3.  This batch measured 1.4e-4 (112) and 3.7e-4 (224)."""
    from devit_amd import engine
    S, s, t, img, soft, dps, ref, grads = hid_step
    loss_bar, norm_bar, slice_bar = (1e-4, 1e-3, 1e-3) if precision == "f32" else (5e-4, 3e-3, 1.5e-2)
    try:
        s.precision = t.precision = precision
        s.train()
        for p in s.parameters():
            p.grad = None
        out = engine.distill_forward(s, t, img.to(dev), soft.to(dev), gama=(0.2, 0.1, 0.3), kind="hard", alpha=0.5, tau=1.0,
                                     dp_scales=[(a.to(dev).contiguous(), b.to(dev).contiguous()) for a, b in dps], hid_gama=0.5)
        fails = []
        for k in ("loss", "cls_loss", "q_loss", "k_loss", "v_loss", "hid_loss"):
            e = abs(float(out[k].detach()) - float(ref[k].detach())) / abs(float(ref[k].detach()))
            print(f"hid step S{S} {precision} {k}: {float(out[k].detach()):.6f} vs {float(ref[k].detach()):.6f} rel {e:.3e}")
            bar = HID_LOSS_BAR if (k == "hid_loss" and precision == "bf16") else loss_bar
            if not chk(e, bar, name=f"hid/step/S{S}/{precision}/{k}"):
                fails.append((k, e))
        out["loss"].backward()
        params = dict(s.named_parameters())
        names = list(params)
        gn = np.array([params[n].grad.norm().item() for n in names])
        rn = np.array([grads[n].norm().item() for n in names])
        if precision == "f32":
            worst = float(np.abs(gn - rn).max() / rn.max())
            if not chk(worst, norm_bar, name=f"hid/step/S{S}/f32/grad_norms"):
                fails.append(("grad norms", worst))
        else:
            chk(float((np.abs(gn - rn) / (rn + 1e-3 * rn.max())).max()), norm_bar, name=f"hid/step/S{S}/bf16/grad_norms")
            bad = np.abs(gn - rn) > norm_bar * rn + 3e-6 * rn.max()
            if bad.any():
                fails.append([(names[i], gn[i], rn[i]) for i in np.nonzero(bad)[0][:8]])
        for n, cut in SLICES:
            e = rel(cut(params[n].grad), cut(grads[n]))
            print(f"hid step S{S} {precision} grad {n}: rel {e:.3e}")
            if not chk(e, slice_bar, name=f"hid/step/S{S}/{precision}/g_{n}"):
                fails.append((n, e))
        assert not fails, fails
    finally:
        s.precision = t.precision = "bf16"
        for p in s.parameters():
            p.grad = None


def test_hid_gama_zero_is_the_step_as_it_was(dev, monkeypatch, hid_step):
    """hid_gama=0: the returned keys, the losses and every gradient are the bits of the call without the argument (one_k_slice: the one sum of the
    step whose order is not fixed gets one)"""
    from devit_amd import engine
    one_k_slice(monkeypatch)
    S, s, t, img, soft, dps, _, _ = hid_step
    x, y = img.to(dev), soft.to(dev)
    d = [(a.to(dev).contiguous(), b.to(dev).contiguous()) for a, b in dps]

    def run(**kw):
        for p in s.parameters():
            p.grad = None
        out = engine.distill_forward(s, t, x, y, gama=(0.2, 0.1, 0.3), dp_scales=d, **kw)
        out["loss"].backward()
        torch.cuda.synchronize()
        return out, {n: p.grad.detach().clone() for n, p in s.named_parameters()}
    s.train()
    o0, g0 = run()
    o1, g1 = run(hid_gama=0.0)
    assert set(o0) == set(o1) == {"loss", "cls_loss", "q_loss", "k_loss", "v_loss", "logits", "teacher_logits"}
    for k in ("loss", "cls_loss", "q_loss", "k_loss", "v_loss"):
        assert torch.equal(o0[k], o1[k]), k
    diff = [n for n in g0 if not torch.equal(g0[n], g1[n])]
    assert not diff, diff
    for p in s.parameters():
        p.grad = None


def test_lookahead_teacher_hands_out_the_hidden_states(dev, hid_step):
    """the look-ahead (side-stream) teacher forward with hid=True: the same hid_loss as the teacher run inside the step"""
    from devit_amd import engine
    S, s, t, img, soft, dps, _, _ = hid_step
    x, y = img.to(dev), soft.to(dev)
    d = [(a.to(dev).contiguous(), b.to(dev).contiguous()) for a, b in dps]
    s.train()
    inside = engine.distill_forward(s, t, x, y, dp_scales=d, hid_gama=0.5)
    look = engine.TeacherLookahead(t, hid=True)
    look.submit(x)
    ahead = engine.distill_forward(s, t, x, y, dp_scales=d, hid_gama=0.5, teacher_outputs=look.take(x))
    assert torch.equal(inside["hid_loss"], ahead["hid_loss"]) and torch.equal(inside["loss"], ahead["loss"])
    plain = engine.TeacherLookahead(t)
    plain.submit(x)
    with pytest.raises(RuntimeError, match="hid=True"):
        engine.distill_forward(s, t, x, y, dp_scales=d, hid_gama=0.5, teacher_outputs=plain.take(x))


# ============================================================================================ the CLI
def test_distill_sub_hid_gama_cli(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import distill_sub
    parser = argparse.ArgumentParser(parents=[distill_sub.get_args_parser()])
    args = parser.parse_args(["--synthetic", "2", "--batch-size", "8", "--input-size", "32", "--epochs", "1", "--hid-gama", "0.3", "--model", "dedeit",
                              "--teacher-model", "deit_base_distilled_patch16_224", "--dataset", "cifar100", "--num_division", "4",
                              "--output_dir", str(tmp_path), "--warmup-epochs", "0"])
    distill_sub.main(args)
    line = json.loads(open(os.path.join(args.output_dir, "sub-dataset0", "log.txt")).read().splitlines()[-1])
    assert np.isfinite(line["train_hid_loss"]) and line["train_hid_loss"] > 0 and np.isfinite(line["train_loss"])
