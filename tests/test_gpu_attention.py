"""csrc/attention.hip against the elementwise error model of tests/_attn_model.py (derived from the inputs: u = 2^-8 for bf16 storage, fp32
eps, the accumulation chain; no fitted factor -- tests/test_attention_model.py shows on the CPU that the bounds hold for an emulation of the
kernels' documented roundings and fail for planted bugs).  O, lse, dQ, dK and dV are each held to their own bound on every element; every
comparison goes through chk(worst |err| / bound, 1.0, name=...), so the measured margins are recorded."""
import math

import pytest
import torch

import _attn_model as A
from conftest import chk

pytestmark = pytest.mark.gpu
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
SCALE = 0.125
SENTINEL = 7.0


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from devit_amd import _lib
    _lib.require_device(torch.zeros(1, device="cuda"))
    return torch.device("cuda")


def padded(x, dev, fill=0.0):
    """a rows_alloc buffer (row count padded to the GEMM tile) holding x in its first rows, `fill` in its pad rows"""
    from devit_amd import ops
    t = ops.rows_alloc(x.shape[0], x.shape[1], x.dtype, dev)
    t[: x.shape[0]] = x.to(dev)
    if fill != 0.0:
        t[x.shape[0]:] = fill
    return t


def fwd_packed(dev, qkv, B, N, H, gate, dtype16=0, out_fill=0.0):
    from devit_amd._lib import call, ptr, stream_ptr
    M, D = B * N, H * 64
    out = padded(torch.zeros((M, D), dtype=qkv.dtype), dev, out_fill)
    lse = torch.full((B * H * N + 64,), SENTINEL, dtype=F32, device=dev)           # 64 floats behind the last row: must stay
    call("devit_attn_fwd", ptr(qkv), ptr(out), ptr(lse), ptr(gate), B, N, H, 64, SCALE, dtype16, stream_ptr())
    torch.cuda.synchronize()
    assert bool((lse[B * H * N:] == SENTINEL).all())
    return out, lse[: B * H * N].view(B, H, N)


def bwd_packed(dev, qkv, out, dout, lse, gate, add, B, N, H):
    from devit_amd._lib import call, ptr, stream_ptr
    dqkv = torch.full((qkv.shape[0], 3 * H * 64), SENTINEL, dtype=BF16, device=dev)
    call("devit_attn_bwd", ptr(qkv), ptr(out), ptr(dout), ptr(lse.contiguous()), ptr(gate), ptr(add), ptr(dqkv), B, N, H, 64, SCALE, stream_ptr())
    torch.cuda.synchronize()
    return dqkv


def case_id(c):
    B, N, H, regime, gated, with_add = c
    return f"B{B}-N{N}-H{H}-{regime}-{'gates' if gated else 'nogate'}-{'add' if with_add else 'noadd'}"


# ------------------------------------------------------------------------------------------ packed forward + backward
@pytest.mark.parametrize("case", A.packed_cases(), ids=case_id)
def test_packed_fwd_bwd_within_model_bounds(dev, case):
    B, N, H, regime, gated, with_add = case
    inp = A.make_inputs(B, N, H, regime)
    M = B * N
    gate = A.gate_mix(H).to(dev) if gated else None
    qkv, dout = padded(inp["qkv"], dev), padded(inp["dout"], dev)
    add = padded(inp["add"], dev) if with_add else None
    out, lse = fwd_packed(dev, qkv, B, N, H, gate, out_fill=SENTINEL)
    assert bool((out[M:] == SENTINEL).all())
    dqkv = bwd_packed(dev, qkv, out, dout, lse, gate, add, B, N, H)
    assert bool((dqkv[M:] == SENTINEL).all())
    A.check_packed(chk, "packed/" + case_id(case), qkv, B, N, H, gate, SCALE, out, lse, dout, dqkv, add)


# ------------------------------------------------------------------------------------------ pad rows
@pytest.mark.parametrize("B,N,H", [(2, 198, 6), (3, 197, 2), (2, 193, 12), (5, 1, 2)])
def test_pad_rows_never_reach_live_rows(dev, B, N, H):
    """Rows >= B N of every INPUT (qkv, dout, dqkv_add, and `out` once the forward has written it) hold NaN: O, lse and dqkv of the live rows
    are finite and the same bits as with zero pad rows -- the kernels clamp their loads to row N - 1 of the image and mask.
    Pad rows of the OUTPUTS: attn_fwd_kernel stores `out` under `qr < NQ` and lse under `q < NQ`; attn_bwd4_kernel stores dQ under
    `q < NQ` and dK / dV under `key < N`, all per image -- so no row >= B N of out, lse or dqkv is ever written: each keeps its sentinel."""
    M = B * N
    inp = A.make_inputs(B, N, H, "unit")
    gate = A.gate_mix(H).to(dev)
    ref = {}
    for fill in (0.0, float("nan")):
        qkv, dout, add = (padded(inp[n], dev, fill) for n in ("qkv", "dout", "add"))
        assert qkv.shape[0] > M
        out, lse = fwd_packed(dev, qkv, B, N, H, gate, out_fill=SENTINEL)
        assert bool((out[M:] == SENTINEL).all())
        out[M:] = fill
        dqkv = bwd_packed(dev, qkv, out, dout, lse, gate, add, B, N, H)
        assert bool((dqkv[M:] == SENTINEL).all())
        got = dict(out=out[:M].clone(), lse=lse.clone(), dqkv=dqkv[:M].clone())
        for n, t in got.items():
            assert bool(torch.isfinite(t.float()).all()), (n, fill)
        if not ref:
            ref = got
    for n in ref:
        assert torch.equal(ref[n], got[n]), n


# ------------------------------------------------------------------------------------------ rows form
ROWS_CASES = [(198, 2, 6, 2), (198, 1, 12, 3), (197, 1, 6, 3), (198, 32, 12, 2), (198, 33, 6, 3), (198, 40, 12, 3), (64, 17, 6, 2),
              (208, 208, 12, 2), (208, 208, 6, 3)]


@pytest.mark.parametrize("N,NQ,H,kvw", ROWS_CASES)
def test_rows_form_within_model_bounds(dev, N, NQ, H, kvw):
    """devit_attn_fwd_rows / devit_attn_bwd_rows against the model (the packed computation with dO zero outside the first NQ query rows), with
    leading dimensions wider than the columns used: q in the first D columns of a [B NQ][3 D] buffer, dq written with ld 3 D, kv / dkv with ld
    2 D (kvw 2) or as columns D.. of a [B N][3 D] buffer (kvw 3).  Every key row of dkv is written, every column outside the ones the kernel owns
    keeps its sentinel, dq has exactly NQ rows per image."""
    from devit_amd._lib import call, ptr, stream_ptr
    B, D = 2, H * 64
    inp = A.make_inputs(B, N, H, "unit" if NQ != 32 else "flat", NQ=NQ)
    gate = A.gate_mix(H).to(dev) if NQ % 2 else None
    qkv = inp["qkv"].to(dev)
    qbuf = torch.full((B * NQ, 3 * D), SENTINEL, dtype=BF16, device=dev)
    qbuf[:, :D] = qkv.view(B, N, 3 * D)[:, :NQ, :D].reshape(B * NQ, D)
    kv = qkv[:, D:].contiguous() if kvw == 2 else qkv[:, D:]                         # kvw 3: a view, row stride 3 D
    kv_ld = kvw * D
    dout = inp["dout"].to(dev)
    out = torch.full((B * NQ + 8, D), SENTINEL, dtype=BF16, device=dev)
    lse = torch.full((B * H * NQ + 64,), SENTINEL, dtype=F32, device=dev)
    call("devit_attn_fwd_rows", ptr(qbuf), 3 * D, ptr(kv), kv_ld, ptr(out), ptr(lse), ptr(gate), B, NQ, N, H, 64, SCALE, 0, stream_ptr())
    torch.cuda.synchronize()
    assert bool((out[B * NQ:] == SENTINEL).all()) and bool((lse[B * H * NQ:] == SENTINEL).all())
    dq = torch.full((B * NQ + 8, 3 * D), SENTINEL, dtype=BF16, device=dev)
    dkv_full = torch.full((B * N + 8, kvw * D), SENTINEL, dtype=BF16, device=dev)
    dkv = dkv_full if kvw == 2 else dkv_full[:, D:]
    call("devit_attn_bwd_rows", ptr(qbuf), 3 * D, ptr(kv), kv_ld, ptr(out), ptr(dout), ptr(lse), ptr(gate), ptr(dq), 3 * D, ptr(dkv), kvw * D,
         B, NQ, N, H, 64, SCALE, stream_ptr())
    torch.cuda.synchronize()
    assert bool((dq[B * NQ:] == SENTINEL).all()) and bool((dq[:, D:] == SENTINEL).all())
    assert bool((dkv_full[B * N:] == SENTINEL).all())
    if kvw == 3:
        assert bool((dkv_full[:, :D] == SENTINEL).all())
    q, k, v = A.heads(qbuf, B, NQ, H), A.heads(qkv, B, N, H, D), A.heads(qkv, B, N, H, 2 * D)
    do = A.heads(dout, B, NQ, H)
    ref, bnd = A.bounds(q, k, v, gate, SCALE, do)
    got = dict(O=A.heads(out, B, NQ, H), lse=lse[: B * H * NQ].double().view(B, H, NQ), dQ=A.heads(dq, B, NQ, H),
               dK=A.heads(dkv, B, N, H, 0), dV=A.heads(dkv, B, N, H, D))
    # (a live element that kept the sentinel fails its bound: 7.0 is far outside every one of them)
    A.check_outputs(chk, f"rows/N{N}-NQ{NQ}-H{H}-kvld{kvw}D", got, ref, bnd)


# ------------------------------------------------------------------------------------------ f16 forward
@pytest.mark.parametrize("B,N,H,regime", [(2, 198, 6, "peaked"), (2, 193, 12, "unit")])
def test_f16_forward_within_model_bounds(dev, B, N, H, regime):
    """dtype16 = 1 (the opt-in teacher path), packed and rows form: u = 2^-10, plus |g| N 2^-25 max|V| for P values that are subnormal in f16."""
    from devit_amd._lib import call, ptr, stream_ptr
    D, NQ = H * 64, 2
    inp = A.make_inputs(B, N, H, regime, dtype=F16)
    gate = A.gate_mix(H).to(dev)
    qkv = padded(inp["qkv"], dev)
    out, lse = fwd_packed(dev, qkv, B, N, H, gate, dtype16=1)
    tag = f"f16/B{B}-N{N}-H{H}-{regime}"
    A.check_packed(chk, tag, qkv, B, N, H, gate, SCALE, out, lse, u=A.U_F16, f16=True)
    q_tok = qkv[: B * N].view(B, N, 3 * D)[:, :NQ, :D].contiguous().view(B * NQ, D)
    kv = qkv[: B * N, D:].contiguous()
    out_r = torch.full((B * NQ, D), SENTINEL, dtype=F16, device=dev)
    lse_r = torch.full((B, H, NQ), SENTINEL, dtype=F32, device=dev)
    call("devit_attn_fwd_rows", ptr(q_tok), D, ptr(kv), 2 * D, ptr(out_r), ptr(lse_r), ptr(gate), B, NQ, N, H, 64, SCALE, 1, stream_ptr())
    torch.cuda.synchronize()
    q, k, v = A.heads(q_tok, B, NQ, H), A.heads(kv, B, N, H, 0), A.heads(kv, B, N, H, D)
    ref, bnd = A.bounds(q, k, v, gate, SCALE, u=A.U_F16, f16=True)
    A.check_outputs(chk, tag + "/rows", dict(O=A.heads(out_r, B, NQ, H), lse=lse_r.double()), ref, bnd)


# ------------------------------------------------------------------------------------------ routing through a saturated softmax
@pytest.mark.parametrize("N", [208, 198, 193, 64, 17])
def test_routing_through_saturated_softmax(dev, N):
    """Q_i = s_i, K_pi(i) = s_i (+-4 sign codes, another permutation per image and head): the matching score is 128, every other <= 72, so P is
    one-hot to 1e-22 and exp(128) overflows fp32 -- a forward that loses the row-max subtraction or a backward that loses the lse cannot pass.
    out == g V[pi(i)] bit for bit (g a power of two), lse = 128, dV[pi(i)] = g dO[i] to 1e-6, dQ / dK within their bounds."""
    B, H = 2, 2
    inp = A.routing_inputs(B, N, H)
    assert inp["max_other"] <= 72
    gate = torch.tensor([2.0, 0.5], device=dev)
    qkv, dout = padded(inp["qkv"], dev), padded(inp["dout"], dev)
    out, lse = fwd_packed(dev, qkv, B, N, H, gate)
    dqkv = bwd_packed(dev, qkv, out, dout, lse, gate, None, B, N, H)
    perm = inp["perm"].to(dev)[..., None].expand(B, H, N, 64)
    g = gate.double().view(1, H, 1, 1)
    v, do = A.heads(qkv, B, N, H, 2 * H * 64), A.heads(dout, B, N, H)
    assert torch.equal(A.heads(out, B, N, H), g * torch.gather(v, 2, perm))
    assert chk(float((lse.double() - 128).abs().max()) / (A.LSE_BAR * 128), 1.0, name=f"routing/N{N}/lse")
    dv_at_pi = torch.gather(A.heads(dqkv, B, N, H, 2 * H * 64), 2, perm)
    assert chk(float((dv_at_pi - g * do).abs().max()), 1e-6, name=f"routing/N{N}/dV_abs")
    A.check_packed(chk, f"routing/N{N}", qkv, B, N, H, gate, SCALE, out, lse, dout, dqkv)


# ------------------------------------------------------------------------------------------ gain
@pytest.mark.parametrize("H", [6, 12])
@pytest.mark.parametrize("regime", ["unit", "flat"])
def test_gain_per_head(dev, H, regime):
    """Least-squares slope of every output against the reference, per head over all images: |slope - 1| <= 2^-9.  Rounding noise is zero-mean;
    a gain error below every max-error bound is not (a dQ scaled by 1.01 passes the bounds and fails this, tests/test_attention_model.py)."""
    B, N = 4, 198
    inp = A.make_inputs(B, N, H, regime)
    gate = A.gate_mix(H, nonzero=True).to(dev)
    qkv, dout = padded(inp["qkv"], dev), padded(inp["dout"], dev)
    out, lse = fwd_packed(dev, qkv, B, N, H, gate)
    dqkv = bwd_packed(dev, qkv, out, dout, lse, gate, None, B, N, H)
    tag = f"gain/H{H}-{regime}"
    A.check_packed(chk, tag, qkv, B, N, H, gate, SCALE, out, lse, dout, dqkv)
    q, k, v, do, _ = A.split_packed(qkv, B, N, H, dout)
    ref = A.reference(q, k, v, gate, SCALE, do)
    D = H * 64
    got = dict(O=A.heads(out, B, N, H), dQ=A.heads(dqkv, B, N, H, 0), dK=A.heads(dqkv, B, N, H, D), dV=A.heads(dqkv, B, N, H, 2 * D))
    worst = {n: float((A.slope(got[n], ref[n]) - 1).abs().max()) for n in got}
    print(tag, worst)
    bad = [n for n, x in worst.items() if not chk(x, A.SLOPE_BAR, name=f"{tag}/slope_{n}")]
    assert not bad, worst
