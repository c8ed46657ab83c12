"""The launches of the lean last block (de_vit.lean_tail -> devit_tail_fwd / devit_tail_bwd), as the library reports them to its launch observer: the
statement that moving the block's host sequence from Python into csrc/encoder.hip changed no launch -- this list was first held against the Python
sequence it replaced.  Two student blocks (D 384, 6 heads, hidden 1536) as one EncoderFn node with lean_tokens = 2, x fp32 [4, 198, 384]: the body
block runs on its M = 792 rows (M_pad 1024), the last block's K, V and LN1 on all rows and everything else on its T = 8 token rows (T_pad 256).
Written out from the shapes: name, operand layouts, epilogue, M N K and split_k of every GEMM, rows / query rows / width and the optional operands
of every LayerNorm and attention launch, the grouped weight-gradient launch's jobs, and the stream -- the caller's, for every one of them."""
import pytest
import torch

pytestmark = pytest.mark.gpu
B, N, NTOK, D, HD = 4, 198, 2, 384, 1536
M, MP, T, TP = B * N, 1024, B * NTOK, 256
STORE, GELU, RESIDUAL, DGELU, ATOMIC = 0, 1, 2, 4, 5
Y_BF16, DRES, DX, DX_BF16 = 1, 8, 16, 32


def gemm(a_km, b_km, kind, m, n, k, split_k=1):
    return ("devit_gemm_bf16", a_km, b_km, kind, m, n, k, split_k, 0, 0, 0, 0, 0, 0)


def wgrad(nw, k, rows):
    """dW[nw][k] += dy^T x over `rows` padded rows: one round of resident 128 x 128 workgroups (csrc/encoder.hip: split_k_for)"""
    return gemm(1, 1, ATOMIC, nw, k, rows, max(1, min(rows // 64, 512 // ((nw // 128) * (k // 128)))))


def ln_fwd(rows):
    return ("devit_layernorm_fwd", 0, 0, 0, 0, 0, 0, 0, rows, D, 0, Y_BF16, 0, 0)


def ln_bwd(rows, has):
    return ("devit_layernorm_bwd", 0, 0, 0, 0, 0, 0, 0, rows, D, 0, has, 0, 0)


def attn(name, q_rows):
    return (name, 0, 0, 0, 0, 0, 0, 0, M, D, q_rows, 0, 0, 0)


def grouped(njobs, a_cols):
    """(its K slices are the kernel's own cost model over the device's CU count, csrc/wgradfr.hip: not a figure of these shapes -- recorded as None)"""
    return ("devit_wgrad_grouped", 1, 1, ATOMIC, 0, 0, MP, None, 0, 0, 0, 0, njobs, a_cols)


def block_fwd(rows):          # from the proj GEMM on: the half the block and the lean last block share
    return [gemm(0, 0, RESIDUAL, rows, D, D), ln_fwd(M if rows == MP else T), gemm(0, 0, GELU, rows, HD, D), gemm(0, 0, RESIDUAL, rows, D, HD)]


FWD = ([ln_fwd(M), gemm(0, 0, STORE, MP, 3 * D, D), attn("devit_attn_fwd", 0)] + block_fwd(MP) +
       # the last block: LN1 and (K | V) on all rows, Q of the token rows, attention of the token rows' queries over all keys
       [ln_fwd(M), gemm(0, 0, STORE, MP, 2 * D, D), gemm(0, 0, STORE, TP, D, D), attn("devit_attn_fwd_rows", T)] + block_fwd(TP))

TAIL_BWD_HEAD = [wgrad(D, HD, TP), gemm(0, 1, DGELU, TP, HD, D), gemm(0, 1, STORE, TP, D, HD), wgrad(HD, D, TP), ln_bwd(T, DRES | DX | DX_BF16),
                 gemm(0, 1, STORE, TP, D, D), wgrad(D, D, TP), attn("devit_attn_bwd_rows", T),
                 gemm(0, 1, STORE, MP, D, 2 * D), gemm(0, 1, STORE, TP, D, 3 * D)]
TAIL_BWD_END = [wgrad(D, D, TP), ln_bwd(M, DX)]
# the body block: its four weight gradients are jobs of the grouped launch behind it (fc2's bias gradient: a column-sum pass, not reported)
BODY_BWD = [gemm(0, 1, DGELU, MP, HD, D), gemm(0, 1, STORE, MP, D, HD), ln_bwd(M, DRES | DX | DX_BF16), gemm(0, 1, STORE, MP, D, D),
            attn("devit_attn_bwd", 0), gemm(0, 1, STORE, MP, D, 3 * D), ln_bwd(M, DRES | DX)]
BODY_JOB_COLS = HD + HD + D + 3 * D
# with a slot for it the (dK | dV)^T ln1 product is the first job of the grouped launch and no launch of its own; without, a split-K launch
BWD_DEFERRED = TAIL_BWD_HEAD + TAIL_BWD_END + BODY_BWD + [grouped(5, 2 * D + BODY_JOB_COLS)]
BWD_LAUNCHED = TAIL_BWD_HEAD + [wgrad(2 * D, D, MP)] + TAIL_BWD_END + BODY_BWD + [grouped(4, BODY_JOB_COLS)]


@pytest.fixture(scope="module")
def setup():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import devit_amd
    dev = torch.device("cuda")
    torch.manual_seed(3)
    blocks = list(devit_amd.create_model("dedeit", num_classes=25, drop_path_rate=0.0).blocks[4:6].to(dev).eval())
    x = torch.randn((B, N, D), generator=torch.Generator().manual_seed(4)).to(dev)
    return blocks, x


def observed(setup, monkeypatch, group):
    from devit_amd import de_vit, ops
    for k in ("DEVIT_GEMMFR", "DEVIT_GEMM_FORCE", "DEVIT_LNFUSE", "DEVIT_WGRADFR", "DEVIT_WGRAD_STREAM"):      # (each is read per call)
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("DEVIT_WGRAD_GROUP", group)
    blocks, x0 = setup
    for b in blocks:
        for p in b.parameters():
            p.grad = None
    x = x0.clone().requires_grad_(True)
    recs = {"fwd": [], "bwd": []}
    cur = torch.cuda.current_stream().cuda_stream
    into = ["fwd"]

    def record(phase, stream, i):
        if phase == 0:
            name = i.name.decode()
            rec = (name, i.a_kmajor, i.b_kmajor, i.kind, i.M, i.N, i.K, None if name == "devit_wgrad_grouped" else i.split_k, i.rows, i.width,
                   i.q_rows, i.has, i.njobs, i.a_cols)
            recs[into[0]].append(rec + (() if (stream or 0) == cur else ("not on the caller's stream",)))
    # The observer is per thread and autograd runs the backward on a thread of its own: ops.call() puts `ops.observing(ops._record)` around every
    # library call while an instrument is set, on whichever thread makes it -- so the instruments' recorder is replaced by this one.
    monkeypatch.setattr(ops, "_record", record)
    monkeypatch.setattr(ops, "PROFILE", [])
    y = de_vit.run_blocks(blocks, x, False, False, False, False, lean_tokens=NTOK)[0]
    assert tuple(y.shape) == (B, NTOK, D)
    into[0] = "bwd"
    y.square().sum().backward()
    fwd, bwd = recs["fwd"], recs["bwd"]
    torch.cuda.synchronize()
    assert tuple(x.grad.shape) == (B, N, D) and bool(torch.isfinite(x.grad).all())
    return fwd, bwd


def diff(got, want):
    return [(k, g, w) for k, (g, w) in enumerate(zip(got + [None] * len(want), want + [None] * len(got))) if g != w]


def test_launches_with_a_slot_for_the_all_rows_weight_gradient(setup, monkeypatch):
    """DEVIT_WGRAD_GROUP=all: the last block rides the encoder's one group; its (dK | dV)^T ln1 product is a job of that launch"""
    fwd, bwd = observed(setup, monkeypatch, "all")
    assert fwd == FWD, diff(fwd, FWD)
    assert bwd == BWD_DEFERRED, diff(bwd, BWD_DEFERRED)


def test_launches_without_a_slot(setup, monkeypatch):
    """DEVIT_WGRAD_GROUP=block: the last block is reported on its own, all five of its weight gradients are split-K launches on the caller's stream"""
    fwd, bwd = observed(setup, monkeypatch, "block")
    assert fwd == FWD, diff(fwd, FWD)
    assert bwd == BWD_LAUNCHED, diff(bwd, BWD_LAUNCHED)
