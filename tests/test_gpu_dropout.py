"""Dropout p > 0 on the HIP path (csrc/dropout.hip, the *_drop kernels of csrc/attention.hip) against the header's mask definition, restated in
numpy by tests/_philox.py, and against fp32 torch statements that use the mask the library dumps (devit_dropout_mask).  The second half of
the file holds the same kernels element by element to the float64 models of tests/_drop_model.py and tests/_attn_model.py (keep, s), with
masks from the numpy mirror only, and the bf16 block path to the statement by the distance of the gradients a wrong backward mask moves."""
import numpy as np
import pytest
import torch

import _attn_model as A
import _drop_model as DM
import _philox as PH
from conftest import chk

pytestmark = pytest.mark.gpu
BF16, F32 = torch.bfloat16, torch.float32
SCALE = 0.125
SEED = 20240807
F32_BAR = 2e-5          # the project's fp32 kernel bar (relative to the largest reference value)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from devit_amd import _lib
    _lib.require_device(torch.zeros(1, device="cuda"))
    return torch.device("cuda")


def lib_mask(dev, seed, site, block, thr, rows, cols, pitch):
    from devit_amd._lib import call, ptr, stream_ptr
    keep = torch.full((rows * cols + 64,), 7, dtype=torch.uint8, device=dev)
    call("devit_dropout_mask", seed, site, block, thr, rows, cols, pitch, ptr(keep), stream_ptr())
    torch.cuda.synchronize()
    assert bool((keep[rows * cols:] == 7).all())
    return keep[: rows * cols].view(rows, cols)


# ------------------------------------------------------------------------------------------ a. the mask definition
@pytest.mark.parametrize("rows,cols,pitch", [(3, 10, 12), (257, 384, 384)])
@pytest.mark.parametrize("site,block", [(0, 0), (4, 0), (4, 11), (0, 11)])
def test_mask_equals_the_numpy_mirror(dev, rows, cols, pitch, site, block):
    for p in (0.1, 0.5):
        thr = PH.threshold(p)
        got = lib_mask(dev, SEED, site, block, thr, rows, cols, pitch).cpu().numpy()
        want = PH.keep_mask(SEED, site, block, thr, rows, cols, pitch)
        assert got.dtype == np.uint8 and set(np.unique(got)) <= {0, 1}
        assert np.array_equal(got.astype(bool), want), (p, int((got.astype(bool) != want).sum()))
    # a 64-bit seed: both key words are used
    seed = (0x9E3779B9 << 32) | 0x12345678
    thr = PH.threshold(0.25)
    got = lib_mask(dev, seed, site, block, thr, rows, cols, pitch).cpu().numpy().astype(bool)
    assert np.array_equal(got, PH.keep_mask(seed, site, block, thr, rows, cols, pitch))
    assert not np.array_equal(got, PH.keep_mask(seed & 0xFFFFFFFF, site, block, thr, rows, cols, pitch))


@pytest.mark.parametrize("p,bar", [(0.1, 1.5e-3), (0.5, 2.5e-3)])
def test_keep_fraction(dev, p, bar):
    """2^20 elements, 5 sigma of a binomial: sqrt(p (1 - p) / 2^20) = 2.9e-4 / 4.9e-4"""
    from devit_amd import dropout
    keep = dropout.keep_mask(SEED, 0, 0, p, 1024, 1024, device=dev)
    frac = float(keep.float().mean())
    print(f"keep fraction p={p}: {frac:.6f} (deviation {abs(frac - (1 - p)):.2e})")
    assert chk(abs(frac - (1 - p)), bar, name=f"dropout/keep_fraction/p{p}")
    assert bool(dropout.keep_mask(SEED, 0, 0, 0.0, 8, 64, device=dev).all())                  # thr == 0 keeps everything


# ------------------------------------------------------------------------------------------ b. the elementwise kernels
@pytest.mark.parametrize("dtype,rows,cols", [(BF16, 257, 384), (BF16, 257, 1536), (F32, 257, 384)])
def test_apply_is_exact_and_its_column_sums_hold(dev, dtype, rows, cols):
    from devit_amd import dropout, ops
    p, site, block = 0.1, 3, 5
    gen = torch.Generator(device="cpu").manual_seed(rows * cols)
    x0 = torch.randn((rows, cols), generator=gen).to(dtype).to(dev)
    buf = ops.rows_alloc(rows, cols, dtype, dev)
    assert buf.shape[0] > rows
    buf[:rows] = x0
    colsum0 = torch.randn(cols, generator=gen).to(dev)
    colsum = colsum0.clone()
    dropout.apply_(buf, rows, SEED, site, block, p, colsum=colsum)
    torch.cuda.synchronize()
    keep = dropout.keep_mask(SEED, site, block, p, rows, cols, pitch=cols, device=dev).bool()
    s = torch.tensor(1.0 / (1.0 - p), dtype=F32, device=dev)
    want = torch.where(keep, x0.float() * s, torch.zeros((), device=dev)).to(dtype)
    assert torch.equal(buf[:rows], want)
    assert bool((buf[rows:] == 0).all())                                       # pad rows: untouched
    ref = colsum0.double() + want.double().sum(0)
    err = float((colsum.double() - ref).abs().max() / ref.abs().max())
    assert chk(err, F32_BAR, name=f"dropout/apply_colsum/{str(dtype)[6:]}-{rows}x{cols}"), err
    # without the accumulator the buffer gets the same bits
    buf2 = ops.rows_alloc(rows, cols, dtype, dev)
    buf2[:rows] = x0
    dropout.apply_(buf2, rows, SEED, site, block, p)
    assert torch.equal(buf2, buf)


def test_apply_with_its_own_ld_and_pitch(dev):
    """a [rows][cols] window of a wider buffer (ld > cols) under a mask pitch > cols, and the 1536-wide mask, against the numpy mirror"""
    from devit_amd import dropout
    from devit_amd._lib import call, ptr, stream_ptr
    rows, cols, ld, pitch, p, site, block = 37, 384, 512, 1536, 0.5, 3, 2
    thr, s = dropout.threshold(p)
    gen = torch.Generator(device="cpu").manual_seed(5)
    x0 = torch.randn((rows, ld), generator=gen).to(BF16).to(dev)
    x = x0.clone()
    call("devit_dropout_apply", ptr(x), 0, rows, cols, ld, pitch, SEED, site, block, thr, s, None, stream_ptr())
    torch.cuda.synchronize()
    keep = torch.from_numpy(PH.keep_mask(SEED, site, block, thr, rows, cols, pitch)).to(dev)
    want = torch.where(keep, x0[:, :cols].float() * torch.tensor(s, dtype=F32, device=dev), torch.zeros((), device=dev)).to(BF16)
    assert torch.equal(x[:, :cols], want) and torch.equal(x[:, cols:], x0[:, cols:])
    wide = dropout.keep_mask(SEED, site, block, p, 257, 1536, pitch=1536, device=dev).cpu().numpy().astype(bool)
    assert np.array_equal(wide, PH.keep_mask(SEED, site, block, thr, 257, 1536, 1536))


def test_residual_against_the_statement(dev):
    from devit_amd import dropout
    rows, cols, rps, p, site, block = 257 * 3, 384, 3, 0.1, 2, 7
    gen = torch.Generator(device="cpu").manual_seed(11)
    x = torch.randn((rows, cols), generator=gen).to(dev)
    y = torch.randn((rows, cols), generator=gen).to(dev)
    rowscale = (torch.rand(rows // rps, generator=gen) > 0.2).float().div(0.8).to(dev)
    keep = dropout.keep_mask(SEED, site, block, p, rows, cols, pitch=cols, device=dev).bool()
    s = 1.0 / (1.0 - p)
    want = x.double() + rowscale.double().repeat_interleave(rps)[:, None] * torch.where(keep, y.double() * s, torch.zeros((), device=dev, dtype=torch.float64))
    got = dropout.residual(x, y, rowscale, rps, SEED, site, block, p)
    torch.cuda.synchronize()
    err = float((got.double() - want).abs().max() / want.abs().max())
    assert chk(err, F32_BAR, name="dropout/residual"), err
    # no DropPath scale, in place over x
    want1 = x.double() + torch.where(keep, y.double() * s, torch.zeros((), device=dev, dtype=torch.float64))
    x1 = x.clone()
    dropout.residual(x1, y, None, 0, SEED, site, block, p, out=x1)
    err = float((x1.double() - want1).abs().max() / want1.abs().max())
    assert chk(err, F32_BAR, name="dropout/residual_in_place"), err


def test_entry_points_refuse_what_they_cannot_do(dev):
    from devit_amd import dropout
    from devit_amd._lib import DevitError
    x = torch.zeros((4, 12), dtype=BF16, device=dev)
    with pytest.raises(DevitError):
        dropout.apply_(x, 4, SEED, 0, 0, 0.1)                                   # 12 columns: not whole 16-byte pieces of bf16
    with pytest.raises(DevitError):
        dropout.keep_mask(SEED, 5, 0, 0.1, 4, 8, device=dev)                    # no such site
    with pytest.raises(DevitError):
        dropout.keep_mask(SEED, 0, 0, 0.1, 4, 10, pitch=10, device=dev)         # pitch % 4
    with pytest.raises(ValueError):
        dropout.keep_mask(SEED, 0, 0, 1.0, 4, 8, device=dev)


# ------------------------------------------------------------------------------------------ attention
def padded(x, dev):
    from devit_amd import ops
    t = ops.rows_alloc(x.shape[0], x.shape[1], x.dtype, dev)
    t[: x.shape[0]] = x.to(dev)
    return t


def attn_run(dev, qkv, dout, gate, B, N, H, drop=None):
    """forward + backward through the C ABI; drop = None (devit_attn_fwd / _bwd) or (seed, block, thr, scale_keep) -> out, lse, dqkv"""
    from devit_amd._lib import call, ptr, stream_ptr
    M, D = B * N, H * 64
    out = padded(torch.zeros((M, D), dtype=BF16), dev)
    lse = torch.full((B * H * N + 64,), 7.0, dtype=F32, device=dev)
    dqkv = torch.full((qkv.shape[0], 3 * D), 7.0, dtype=BF16, device=dev)
    if drop is None:
        call("devit_attn_fwd", ptr(qkv), ptr(out), ptr(lse), ptr(gate), B, N, H, 64, SCALE, 0, stream_ptr())
        call("devit_attn_bwd", ptr(qkv), ptr(out), ptr(dout), ptr(lse), ptr(gate), None, ptr(dqkv), B, N, H, 64, SCALE, stream_ptr())
    else:
        seed, block, thr, s = drop
        call("devit_attn_fwd_drop", ptr(qkv), ptr(out), ptr(lse), ptr(gate), B, N, H, 64, SCALE, seed, block, thr, s, stream_ptr())
        call("devit_attn_bwd_drop", ptr(qkv), ptr(out), ptr(dout), ptr(lse), ptr(gate), None, ptr(dqkv), B, N, H, 64, SCALE, seed, block, thr, s,
             stream_ptr())
    torch.cuda.synchronize()
    assert bool((lse[B * H * N:] == 7.0).all()) and bool((dqkv[M:] == 7.0).all()) and bool((out[M:] == 0).all())
    return out, lse[: B * H * N].clone(), dqkv


@pytest.mark.parametrize("B,H,N", [(2, 2, 198), (1, 1, 208)])
def test_attention_thr0_is_bit_identical_to_the_plain_kernels(dev, B, H, N):
    """thr == 0 drops nothing and scale_keep == 1: the *_drop kernels are the plain kernels' arithmetic with the mask lines in it"""
    inp = A.make_inputs(B, N, H, "unit")
    gate = A.gate_mix(H, nonzero=True).to(dev)
    qkv, dout = padded(inp["qkv"], dev), padded(inp["dout"], dev)
    out0, lse0, dqkv0 = attn_run(dev, qkv, dout, gate, B, N, H)
    out1, lse1, dqkv1 = attn_run(dev, qkv, dout, gate, B, N, H, drop=(SEED, 3, 0, 1.0))
    assert torch.equal(out0, out1) and torch.equal(lse0, lse1) and torch.equal(dqkv0, dqkv1)


def attn_statement(qkv, dout, gate, keep, s, B, N, H):
    """fp32 torch: softmax(q k^T scale) -> * keep * s -> @ v -> head gate, and autograd's gradients; heads form [B][H][N][64]"""
    D = H * 64
    t = qkv[: B * N].float().view(B, N, 3, H, 64).permute(2, 0, 3, 1, 4).contiguous().requires_grad_(True)
    q, k, v = t[0], t[1], t[2]
    P = torch.softmax((q @ k.transpose(-1, -2)) * SCALE, dim=-1)
    if keep is not None:
        P = P * (keep.view(B, H, N, N).float() * s)
    o = (P @ v) * gate.view(1, H, 1, 1)
    out = o.permute(0, 2, 1, 3).reshape(B * N, D)
    (g,) = torch.autograd.grad(out, t, dout[: B * N].float())
    dqkv = g.permute(1, 3, 0, 2, 4).reshape(B * N, 3 * D)
    return out.detach(), dqkv


def deviations(out, dqkv, ref_out, ref_dqkv, M, D):
    d = {"out": float((out[:M].float() - ref_out).abs().max())}
    for j, n in enumerate(("dq", "dk", "dv")):
        d[n] = float((dqkv[:M, j * D:(j + 1) * D].float() - ref_dqkv[:, j * D:(j + 1) * D]).abs().max())
    return d


@pytest.mark.parametrize("B,H,N", [(2, 2, 198), (1, 1, 208), (1, 2, 5)])
def test_attention_dropout_against_the_fp32_statement(dev, B, H, N):
    """out, dq, dk, dv under p = 0.1 and 0.5 against the fp32 statement with the library's own mask.  Bar: the plain kernels' deviation from
    the same statement without a mask, measured here on the same inputs, times 1 / (1 - p) (dropout scales P by it and removes terms; it adds no
    rounding step) times a margin of 2.  The ragged last key tile (198), thirteen full tiles (208) and one partial tile (5)."""
    from devit_amd import dropout
    M, D = B * N, H * 64
    inp = A.make_inputs(B, N, H, "unit")
    gate = A.gate_mix(H, nonzero=True).to(dev)
    qkv, dout = padded(inp["qkv"], dev), padded(inp["dout"], dev)
    out0, lse0, dqkv0 = attn_run(dev, qkv, dout, gate, B, N, H)
    base = deviations(out0, dqkv0, *attn_statement(qkv, dout, gate, None, 1.0, B, N, H), M, D)
    print(f"attention B{B} H{H} N{N} p=0: {base}")
    bad = []
    for p in (0.1, 0.5):
        thr, s = dropout.threshold(p)
        block = 4
        keep = dropout.keep_mask(SEED, 1, block, p, B * H * N, N, device=dev)              # pitch ceil4(N)
        assert 0 < int(keep.sum()) < keep.numel()
        out, lse, dqkv = attn_run(dev, qkv, dout, gate, B, N, H, drop=(SEED, block, thr, s))
        assert torch.equal(lse, lse0)                                                       # the log-sum-exp is of the undropped row
        got = deviations(out, dqkv, *attn_statement(qkv, dout, gate, keep, np.float32(s).item(), B, N, H), M, D)
        print(f"attention B{B} H{H} N{N} p={p}: {got}")
        for n in got:
            if not chk(got[n], 2.0 / (1.0 - p) * base[n], name=f"dropout/attention/B{B}-H{H}-N{N}/p{p}/{n}"):
                bad.append((p, n, got[n], base[n]))
    assert not bad, bad


def test_dropped_pairs_contribute_exactly_zero_to_dv(dev):
    """Zeroing row q0 of dout removes query q0's term P[q0][k] keep s dO[q0] from dV[k]: for the keys q0 dropped that term was exactly zero, so
    their dV rows keep their bits; the keys it kept change."""
    from devit_amd import dropout
    B, H, N, p, block, q0 = 1, 2, 198, 0.5, 2, 37
    D = H * 64
    inp = A.make_inputs(B, N, H, "unit")
    gate = A.gate_mix(H, nonzero=True).to(dev)
    qkv, dout = padded(inp["qkv"], dev), padded(inp["dout"], dev)
    thr, s = dropout.threshold(p)
    keep = dropout.keep_mask(SEED, 1, block, p, B * H * N, N, device=dev).view(B, H, N, N).bool()
    # the forward's out for the full dout serves both: delta of the rows other than q0 does not change
    _, _, dqkv_a = attn_run(dev, qkv, dout, gate, B, N, H, drop=(SEED, block, thr, s))
    dout_b = dout.clone()
    dout_b[q0] = 0
    _, _, dqkv_b = attn_run(dev, qkv, dout_b, gate, B, N, H, drop=(SEED, block, thr, s))
    for h in range(H):
        dv_a, dv_b = (t[:N, 2 * D + h * 64: 2 * D + (h + 1) * 64] for t in (dqkv_a, dqkv_b))
        same = (dv_a == dv_b).all(dim=1)
        dropped = ~keep[0, h, q0]
        assert 0 < int(dropped.sum()) < N
        assert bool(same[dropped].all()), h
        assert bool((~same[~dropped]).any()), h


# ------------------------------------------------------------------------------------------ e, f, g: the model
MODEL_SEED = 0x5EED5EED1234


def make_model(dev, precision, drop=0.1, attn_drop=0.1, drop_path=0.1, seed=MODEL_SEED):
    import devit_amd
    torch.manual_seed(1234)
    m = devit_amd.create_model("dedeit", depth=2, num_classes=10, drop_rate=drop, attn_drop_rate=attn_drop, drop_path_rate=drop_path)
    m.precision = precision
    m.dropout_seed = seed
    return m.to(dev).train()


@pytest.fixture(scope="module")
def model_case(dev):
    """the f32-mode model's logits and gradients for one pinned seed, with the DropPath scales it drew; shared by e and f, left unchanged"""
    from devit_amd import de_vit
    gen = torch.Generator(device="cpu").manual_seed(99)
    img = torch.randn((4, 3, 224, 224), generator=gen).to(dev)
    w = (torch.randn((2, 4, 10), generator=gen)).to(dev)
    m = make_model(dev, "f32")
    drawn = []
    orig = de_vit.draw_dp_scales

    def recording(*a, **k):
        r = orig(*a, **k)
        drawn.append(r)
        return r
    de_vit.draw_dp_scales = recording
    try:
        torch.manual_seed(7)
        lo, lk = m(img)
    finally:
        de_vit.draw_dp_scales = orig
    ((lo * w[0]).sum() + (lk * w[1]).sum()).backward()
    torch.cuda.synchronize()
    grads = {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}
    return dict(img=img, w=w, state={k: v.detach().clone() for k, v in m.state_dict().items()}, dps=drawn[0],
                logits=(lo.detach().clone(), lk.detach().clone()), grads=grads)


def torch_statement(state, img, dps, seed, p, p_attn, dev):
    """models/de_vit.py:35-121 and the model around it as plain fp32 torch, with the library's masks and the recorded DropPath scales"""
    from devit_amd import dropout
    F = torch.nn.functional
    P = {k: v.clone().requires_grad_(True) for k, v in state.items()}
    B, D, H, N = img.shape[0], 384, 6, 198
    s, s_a = 1.0 / (1.0 - p), 1.0 / (1.0 - p_attn)

    def keep(site, block, pp, rows, cols, shape):
        return dropout.keep_mask(seed, site, block, pp, rows, cols, device=dev).view(shape).float()
    x = F.conv2d(img, P["patch_embed.proj.weight"], P["patch_embed.proj.bias"], stride=16).flatten(2).transpose(1, 2)
    x = torch.cat((P["cls_token"].expand(B, -1, -1), P["dist_token"].expand(B, -1, -1), x), dim=1) + P["pos_embed"]
    x = x * keep(0, 0, p, B * N, D, (B, N, D)) * s
    for i in range(2):
        g = lambda n: P[f"blocks.{i}.{n}"]
        dp1, dp2 = dps[i] if dps is not None and dps[i] is not None else (torch.ones(B, device=dev),) * 2
        h = F.layer_norm(x, (D,), g("norm1.weight"), g("norm1.bias"), 1e-6)
        qkv = F.linear(h, g("attn.qkv.weight"), g("attn.qkv.bias")).reshape(B, N, 3, H, 64).permute(2, 0, 3, 1, 4)
        q, k, v = qkv[0], qkv[1], qkv[2]
        a = ((q @ k.transpose(-2, -1)) * 0.125).softmax(dim=-1)
        a = a * keep(1, i, p_attn, B * H * N, N, (B, H, N, N)) * s_a
        o = (a @ v).transpose(1, 2).reshape(B, N, D)
        y = F.linear(o, g("attn.proj.weight"), g("attn.proj.bias")) * keep(2, i, p, B * N, D, (B, N, D)) * s
        x = x + dp1.view(B, 1, 1) * y
        h = F.layer_norm(x, (D,), g("norm2.weight"), g("norm2.bias"), 1e-6)
        h = F.gelu(F.linear(h, g("mlp.fc1.weight"), g("mlp.fc1.bias"))) * keep(3, i, p, B * N, 1536, (B, N, 1536)) * s
        y = F.linear(h, g("mlp.fc2.weight"), g("mlp.fc2.bias")) * keep(4, i, p, B * N, D, (B, N, D)) * s
        x = x + dp2.view(B, 1, 1) * y
    x = F.layer_norm(x, (D,), P["norm.weight"], P["norm.bias"], 1e-6)
    return F.linear(x[:, 0], P["head.weight"], P["head.bias"]), F.linear(x[:, 1], P["head_dist.weight"], P["head_dist.bias"]), P


def relmax(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30))


def test_f32_model_against_the_torch_statement(dev, model_case):
    """e: logits and every parameter gradient of the precision="f32" model at 1e-4 (that mode's bar against the oracle)"""
    c = model_case
    lo, lk, P = torch_statement(c["state"], c["img"], c["dps"], MODEL_SEED, 0.1, 0.1, dev)
    ((lo * c["w"][0]).sum() + (lk * c["w"][1]).sum()).backward()
    worst = {"logits": max(relmax(c["logits"][0], lo.detach()), relmax(c["logits"][1], lk.detach()))}
    assert set(c["grads"]) == {n for n, t in P.items() if t.grad is not None}
    for n, gr in c["grads"].items():
        worst[n] = relmax(gr, P[n].grad.view_as(gr))
    top = sorted(worst.items(), key=lambda kv: -kv[1])[:5]
    print("f32 model vs torch statement, worst:", top)
    bad = [(n, v) for n, v in worst.items() if not chk(v, 1e-4, name=f"dropout/model_f32/{n}")]
    assert not bad, bad


def test_bf16_model_against_the_f32_mode(dev, model_case):
    """f: same weights, seed and DropPath scales on the 16-bit path: logits within 3e-2 of max |logit|, gradient norms within 6e-2
    (the statistic of tests/test_gpu_model.py: |norm - ref| / (ref + 1e-3 max ref))"""
    from devit_amd import de_vit
    c = model_case
    m = make_model(dev, "bf16")
    m.load_state_dict(c["state"])
    orig = de_vit.draw_dp_scales
    de_vit.draw_dp_scales = lambda *a, **k: c["dps"]
    try:
        lo, lk = m(c["img"])
    finally:
        de_vit.draw_dp_scales = orig
    ((lo * c["w"][0]).sum() + (lk * c["w"][1]).sum()).backward()
    torch.cuda.synchronize()
    ref = torch.cat(c["logits"])
    err = float((torch.cat((lo, lk)).detach() - ref).abs().max() / ref.abs().max())
    print("bf16 vs f32 logits:", err)
    assert chk(err, 3e-2, name="dropout/model_bf16/logits"), err
    names = sorted(c["grads"])
    params = dict(m.named_parameters())
    gn = torch.stack([params[n].grad.norm() for n in names]).double()
    gr = torch.stack([c["grads"][n].norm() for n in names]).double()
    stat = (gn - gr).abs() / (gr + 1e-3 * gr.max())
    i = int(stat.argmax())
    print("bf16 vs f32 gradient norms, worst:", names[i], float(stat[i]))
    assert chk(float(stat.max()), 6e-2, name="dropout/model_bf16/grad_norms"), (names[i], float(stat[i]))


@pytest.mark.parametrize("precision", ["bf16", "f32"])
def test_switches(dev, model_case, precision):
    """g: eval() with the rates set is bit-identical to a drop_rate = 0 model; a pinned seed reproduces bit for bit, another seed differs;
    dropout_seed = None reproduces under torch.manual_seed"""
    c = model_case
    img = c["img"]
    m = make_model(dev, precision, drop_path=0.0)
    m0 = make_model(dev, precision, drop=0.0, attn_drop=0.0, drop_path=0.0)
    sd = {k: v for k, v in c["state"].items()}
    m.load_state_dict(sd)
    m0.load_state_dict(sd)
    with torch.no_grad():
        assert torch.equal(m.eval()(img), m0.eval()(img))
        m.train()
        a, b = m(img), m(img)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        assert not torch.equal(a[0], m0.train()(img)[0])                      # ... and dropout does run
        m.dropout_seed = MODEL_SEED + 1
        assert not torch.equal(m(img)[0], a[0])
        m.dropout_seed = None
        torch.manual_seed(0)
        x = m(img)
        y = m(img)
        torch.manual_seed(0)
        z = m(img)
        assert torch.equal(x[0], z[0]) and torch.equal(x[1], z[1]) and not torch.equal(x[0], y[0])


# ========================================================================================== per-element bounds (tests/_drop_model.py,
# the keep / s arguments of tests/_attn_model.py): masks from the numpy mirror only, never from devit_dropout_mask
GUARD = 64


def guarded(payload, dev, fill=7):
    """-> (whole buffer, the payload's view): GUARD elements of `fill` on either side of a flat copy of `payload` (256 / 128 / 64 bytes:
    the payload stays 16-byte aligned)"""
    n = payload.numel()
    whole = torch.full((n + 2 * GUARD,), fill, dtype=payload.dtype, device=dev)
    whole[GUARD:GUARD + n] = payload.reshape(-1).to(dev)
    return whole, whole[GUARD:GUARD + n]


def guards_intact(whole, fill=7):
    return bool((whole[:GUARD] == fill).all()) and bool((whole[-GUARD:] == fill).all())


def judged(tag, res):
    print(tag, res)
    bad = [n for n, x in res.items() if not chk(x, 1.0, name=f"{tag}/{n}")]
    assert not bad, (tag, res)


@pytest.mark.parametrize("case", [c["name"] for c in DM.MASK_CASES])
def test_mask_cases_equal_the_mirror(dev, case):
    from devit_amd._lib import call, ptr, stream_ptr
    c = DM.CASES["mask/" + case]
    whole, keep = guarded(torch.full((c["rows"] * c["cols"],), 7, dtype=torch.uint8), dev)
    call("devit_dropout_mask", c["seed"], c["site"], c["block"], DM.thr_s(c["p"])[0], c["rows"], c["cols"], c["pitch"], ptr(keep), stream_ptr())
    torch.cuda.synchronize()
    assert guards_intact(whole)
    judged("dropout_bounds/mask/" + case, DM.judge_mask(c, keep.view(c["rows"], c["cols"]).cpu()))


@pytest.mark.parametrize("case", [c["name"] for c in DM.APPLY_CASES])
def test_apply_cases_against_the_model(dev, case):
    from devit_amd._lib import call, ptr, stream_ptr
    c = DM.CASES["apply/" + case]
    inp = DM.inputs(c)
    thr, s = DM.thr_s(c["p"])
    xw, x = guarded(inp["x"], dev)
    cw, colsum = guarded(inp["colsum0"], dev)
    call("devit_dropout_apply", ptr(x), 1 if c["dtype"] == F32 else 0, c["rows"], c["cols"], c["ld"], c["pitch"], c["seed"], c["site"], c["block"],
         thr, s, ptr(colsum) if c["colsum"] else None, stream_ptr())
    torch.cuda.synchronize()
    assert guards_intact(xw) and guards_intact(cw)
    if not c["colsum"]:
        assert torch.equal(colsum.cpu(), inp["colsum0"])
    judged("dropout_bounds/apply/" + case, DM.judge_apply(c, inp, x.view(c["rows"], c["ld"]).cpu(), colsum.cpu() if c["colsum"] else None))


@pytest.mark.parametrize("case", [c["name"] for c in DM.RESIDUAL_CASES])
def test_residual_cases_against_the_model(dev, case):
    from devit_amd._lib import call, ptr, stream_ptr
    c = DM.CASES["residual/" + case]
    inp = DM.inputs(c)
    thr, s = DM.thr_s(c["p"])
    xw, x = guarded(inp["x"], dev)
    yw, y = guarded(inp["y"], dev)
    ow, out = (xw, x) if c["in_place"] else guarded(torch.full_like(inp["x"], 7.0), dev)
    rs = None if inp["rowscale"] is None else inp["rowscale"].to(dev)
    call("devit_dropout_residual", ptr(x), ptr(y), ptr(out), ptr(rs), c["rps"], c["rows"], c["cols"], c["seed"], c["site"], c["block"], thr, s,
         stream_ptr())
    torch.cuda.synchronize()
    assert guards_intact(xw) and guards_intact(yw) and guards_intact(ow)
    assert torch.equal(y.cpu(), inp["y"].reshape(-1)) and (c["in_place"] or torch.equal(x.cpu(), inp["x"].reshape(-1)))
    judged("dropout_bounds/residual/" + case, DM.judge_residual(c, inp, out.view(c["rows"], c["cols"]).cpu()))


@pytest.mark.parametrize("B,N,H,regime,gated,with_add,p,block", A.DROP_CASES)
def test_dropped_attention_against_the_bounds(dev, B, N, H, regime, gated, with_add, p, block):
    """devit_attn_fwd_drop / devit_attn_bwd_drop, every element of out, dq, dk, dv against _attn_model.bounds(..., keep, s) with keep from the
    numpy mirror; lse has the plain kernels' bits; a head gated off is exactly 0 (its bound is)"""
    from devit_amd._lib import call, ptr, stream_ptr
    M, D = B * N, H * 64
    inp = A.make_inputs(B, N, H, regime)
    gate = (A.gate_mix(H) if gated else torch.ones(H)).to(dev)
    thr, s = A.drop_params(p)
    keep = A.attn_keep(A.DROP_SEED, block, thr, B, H, N)
    qkv, dout = padded(inp["qkv"], dev), padded(inp["dout"], dev)
    add = padded(inp["add"], dev) if with_add else None
    out = padded(torch.zeros((M, D), dtype=BF16), dev)
    lw, lse = guarded(torch.full((B * H * N,), 7.0), dev, fill=7.0)
    lse0 = torch.empty_like(lse)
    dqkv = torch.full((qkv.shape[0], 3 * D), 7.0, dtype=BF16, device=dev)
    call("devit_attn_fwd", ptr(qkv), ptr(out), ptr(lse0), ptr(gate), B, N, H, 64, SCALE, 0, stream_ptr())
    out.zero_()
    call("devit_attn_fwd_drop", ptr(qkv), ptr(out), ptr(lse), ptr(gate), B, N, H, 64, SCALE, A.DROP_SEED, block, thr, s, stream_ptr())
    call("devit_attn_bwd_drop", ptr(qkv), ptr(out), ptr(dout), ptr(lse), ptr(gate), ptr(add), ptr(dqkv), B, N, H, 64, SCALE, A.DROP_SEED, block,
         thr, s, stream_ptr())
    torch.cuda.synchronize()
    assert guards_intact(lw, 7.0) and bool((dqkv[M:] == 7.0).all()) and bool((out[M:] == 0).all())
    assert torch.equal(lse, lse0)
    A.check_packed(chk, f"dropout_bounds/attention/B{B}-N{N}-H{H}-{regime}-p{p}-blk{block}" + ("-add" if with_add else ""), qkv.cpu(), B, N, H,
                   gate.cpu() if gated else None, SCALE, out.cpu(), lse.cpu(), dout.cpu(), dqkv.cpu(), add.cpu() if with_add else None,
                   keep=keep, s=s)


# ------------------------------------------------------------------------------------------ a backward must use its forward's mask
class _MaskFn(torch.autograd.Function):
    """x * m_fwd forward, dy * m_bwd backward: a backward that regenerated another mask than its forward used"""
    @staticmethod
    def forward(ctx, x, m_fwd, m_bwd):
        ctx.save_for_backward(m_bwd)
        return x * m_fwd

    @staticmethod
    def backward(ctx, dy):
        return dy * ctx.saved_tensors[0], None, None


_MIRROR = {}          # the mirror's masks of one model forward, generated once (read-only)


def mirror_statement(state, img, dps, seed, p, p_attn, dev, wrong=None):
    """torch_statement() with the masks of the numpy mirror; wrong = (site, block): that site's BACKWARD takes block + 1's mask"""
    F = torch.nn.functional
    P = {k: v.clone().requires_grad_(True) for k, v in state.items()}
    B, D, H, N = img.shape[0], 384, 6, 198
    s, s_a = float(np.float32(1.0 / (1.0 - p))), float(np.float32(1.0 / (1.0 - p_attn)))

    def mirror(site, block, pp, rows, cols):
        key = (seed, site, block, pp, rows, cols, str(dev))
        if key not in _MIRROR:
            _MIRROR[key] = torch.from_numpy(PH.keep_mask(seed, site, block, PH.threshold(pp), rows, cols, (cols + 3) & ~3)).to(dev).float()
        return _MIRROR[key]

    def drop(x, site, block, pp, sc, rows, cols):
        m = mirror(site, block, pp, rows, cols).view(x.shape) * sc
        if wrong == (site, block):
            return _MaskFn.apply(x, m, mirror(site, block + 1, pp, rows, cols).view(x.shape) * sc)
        return x * m
    x = F.conv2d(img, P["patch_embed.proj.weight"], P["patch_embed.proj.bias"], stride=16).flatten(2).transpose(1, 2)
    x = torch.cat((P["cls_token"].expand(B, -1, -1), P["dist_token"].expand(B, -1, -1), x), dim=1) + P["pos_embed"]
    x = drop(x, 0, 0, p, s, B * N, D)
    for i in range(2):
        g = lambda n: P[f"blocks.{i}.{n}"]
        dp1, dp2 = dps[i] if dps is not None and dps[i] is not None else (torch.ones(B, device=dev),) * 2
        h = F.layer_norm(x, (D,), g("norm1.weight"), g("norm1.bias"), 1e-6)
        qkv = F.linear(h, g("attn.qkv.weight"), g("attn.qkv.bias")).reshape(B, N, 3, H, 64).permute(2, 0, 3, 1, 4)
        q, k, v = qkv[0], qkv[1], qkv[2]
        a = drop(((q @ k.transpose(-2, -1)) * 0.125).softmax(dim=-1), 1, i, p_attn, s_a, B * H * N, N)
        o = (a @ v).transpose(1, 2).reshape(B, N, D)
        y = drop(F.linear(o, g("attn.proj.weight"), g("attn.proj.bias")), 2, i, p, s, B * N, D)
        x = x + dp1.view(B, 1, 1) * y
        h = F.layer_norm(x, (D,), g("norm2.weight"), g("norm2.bias"), 1e-6)
        h = drop(F.gelu(F.linear(h, g("mlp.fc1.weight"), g("mlp.fc1.bias"))), 3, i, p, s, B * N, 1536)
        y = drop(F.linear(h, g("mlp.fc2.weight"), g("mlp.fc2.bias")), 4, i, p, s, B * N, D)
        x = x + dp2.view(B, 1, 1) * y
    x = F.layer_norm(x, (D,), P["norm.weight"], P["norm.bias"], 1e-6)
    return F.linear(x[:, 0], P["head.weight"], P["head.bias"]), F.linear(x[:, 1], P["head_dist.weight"], P["head_dist.bias"]), P


def rel_l2(a, b):
    return float((a.double() - b.double().view_as(a)).norm() / b.double().norm().clamp_min(1e-300))


WITNESS_FLOOR = 0.05


def test_bf16_block_path_backward_uses_its_forwards_masks(dev, model_case):
    """The bf16 model (devit_encoder_fwd_drop / devit_block_bwd_drop) against the fp32 torch statement fed the numpy mirror's masks, by the
    relative L2 DISTANCE of every witness gradient.  The bar comes from the statement alone: for each site and block the statement is run
    once more with that site's backward mask taken from block + 1; d_wrong is that run's distance from the right statement, per
    parameter tensor.  A site's witnesses are the three (block, tensor) pairs with the largest d_wrong, chosen so that every block has
    one: each block's largest first, then the largest of the rest.  Every witness must have d_wrong >= 0.05, and the model must stay below
    d_wrong / 3 on it.  Site 0 (pos_drop) exists once, at block 0.  (The attention mask moves only what lies before the softmax of its
    own block: two tensors per block by more than 0.05, which is why the three are taken per site and not per block.)"""
    from devit_amd import de_vit
    c = model_case
    w = c["w"]

    def grads_of(wrong=None):
        lo, lk, P = mirror_statement(c["state"], c["img"], c["dps"], MODEL_SEED, 0.1, 0.1, dev, wrong)
        ((lo * w[0]).sum() + (lk * w[1]).sum()).backward()
        return {n: t.grad.detach() for n, t in P.items() if t.grad is not None}
    right = grads_of()
    m = make_model(dev, "bf16")
    m.load_state_dict(c["state"])
    orig = de_vit.draw_dp_scales
    de_vit.draw_dp_scales = lambda *a, **k: c["dps"]
    try:
        lo, lk = m(c["img"])
    finally:
        de_vit.draw_dp_scales = orig
    ((lo * w[0]).sum() + (lk * w[1]).sum()).backward()
    torch.cuda.synchronize()
    model = {n: p.grad.detach() for n, p in m.named_parameters() if p.grad is not None}
    assert set(model) == set(right)
    d_model = {n: rel_l2(model[n], right[n]) for n in right}
    bad = []
    for site in range(5):
        runs = {}
        for block in ((0,) if site == 0 else (0, 1)):
            wrong = grads_of((site, block))
            runs[block] = {n: rel_l2(wrong[n], right[n]) for n in right}
        pairs = sorted(((d, b, n) for b, dw in runs.items() for n, d in dw.items()), reverse=True)
        witnesses = [max(p for p in pairs if p[1] == b) for b in runs]
        witnesses += [p for p in pairs if p not in witnesses][:3 - len(witnesses)]
        assert len(witnesses) == 3 and {b for _, b, _ in witnesses} == set(runs)
        for d_wrong, block, n in witnesses:
            print(f"site {site} block {block} witness {n}: d_wrong {d_wrong:.4f} d_model {d_model[n]:.4f}")
            assert d_wrong >= WITNESS_FLOOR, (site, block, n, d_wrong)
            if not chk(d_model[n], d_wrong / 3.0, name=f"dropout_bounds/block_path/site{site}-blk{block}/{n}"):
                bad.append((site, block, n, d_model[n], d_wrong))
    assert not bad, bad
