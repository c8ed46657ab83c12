"""bench.py's instruments (ops.PROFILE / PROFILE_HBM / PROFILE_WGRAD) on the library's launch observer (devit_set_launch_observer): the
instrumented step is the step that runs -- same results -- and its records are the launches csrc/encoder.hip enqueues, no more, no fewer.

One student block: blocks[5] of dedeit (D 384, 6 heads, hidden 1536) in eval mode (no DropPath draw), x fp32 [2, 198, 384]: M = 396 token rows,
M_pad = 512.  The expected launches are read off devit_encoder_fwd / devit_block_bwd for a single (= topmost and lowest) block whose four weight
gradients ride one grouped launch."""
import collections

import pytest
import torch

from conftest import chk

pytestmark = pytest.mark.gpu
B, N, D, HD = 2, 198, 384, 1536
M, MP = B * N, 512

FWD = [("A_row/B_row", MP, 3 * D, D, 1), ("A_row/B_row", MP, D, D, 1), ("A_row/B_row", MP, HD, D, 1), ("A_row/B_row", MP, D, HD, 1)]
HBM_FWD = [("layernorm_fwd", M * D * 6)] * 2 + [("attention_fwd", M * D * 8)]
WGRAD = [(2.0 * MP * 4608 * D, MP * (4608 + 4 * D) * 2 + 4608 * D * 4)]          # four jobs, a_cols 1536 + 1536 + 384 + 1152


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda")


@pytest.fixture(scope="module")
def block(dev):
    import devit_amd
    torch.manual_seed(3)
    blk = devit_amd.create_model("dedeit", num_classes=25, drop_path_rate=0.1).blocks[5].to(dev).eval()
    x = torch.randn((B, N, D), generator=torch.Generator().manual_seed(4)).to(dev)
    return blk, x


def run(block, lists=False):
    """One forward + backward of the block; lists: with the three instruments set.  Returns y, x.grad, the parameter gradients, the records."""
    from devit_amd import ops
    blk, x0 = block
    for p in blk.parameters():
        p.grad = None
    x = x0.clone().requires_grad_(True)
    try:
        if lists:
            ops.PROFILE, ops.PROFILE_HBM, ops.PROFILE_WGRAD = [], [], []
        y = blk(x)["output"]
        y.square().sum().backward()
        torch.cuda.synchronize()
        recs = (ops.PROFILE, ops.PROFILE_HBM, ops.PROFILE_WGRAD)
    finally:
        ops.PROFILE = ops.PROFILE_HBM = ops.PROFILE_WGRAD = None
    grads = {n: p.grad.detach().clone() for n, p in blk.named_parameters()}
    for p in blk.parameters():
        p.grad = None
    return y.detach(), x.grad.detach(), grads, recs


def default_env(monkeypatch):
    for k in ("DEVIT_GEMMFR", "DEVIT_GEMM_FORCE", "DEVIT_LNFUSE", "DEVIT_WGRADFR", "DEVIT_WGRAD_GROUP"):      # (each is read per call)
        monkeypatch.delenv(k, raising=False)


@pytest.fixture(scope="module")
def plain(block):
    """The uninstrumented run in the default environment: computed once, compared against by every test below."""
    with pytest.MonkeyPatch.context() as mp:
        default_env(mp)
        return run(block)


def check_records(recs, gemm_bwd, hbm_bwd):
    prof, hbm, wg = recs
    assert collections.Counter(r[:5] for r in prof) == collections.Counter(FWD + gemm_bwd), [r[:5] for r in prof]
    assert collections.Counter(r[:2] for r in hbm) == collections.Counter(HBM_FWD + hbm_bwd), [r[:2] for r in hbm]
    assert [r[:2] for r in wg] == WGRAD, [r[:2] for r in wg]
    for r in prof + hbm + wg:
        assert r[-2].elapsed_time(r[-1]) > 0, r[:-2]


def test_instrumented_run_equals_plain_run(block, plain, monkeypatch):
    default_env(monkeypatch)
    y0, dx0, g0, _ = plain
    y1, dx1, g1, _ = run(block, lists=True)
    assert torch.equal(y0, y1) and torch.equal(dx0, dx1)
    for n in g0:          # (weight gradients: fp32 atomics, summation order only)
        assert chk(float((g1[n] - g0[n]).abs().max() / g0[n].abs().max()), 2e-5), n


def test_records_default(block, monkeypatch):
    """Nothing forced: at 2 row tiles the full-row kernel is not selected, every dgrad and every LayerNorm backward is a launch of its own."""
    default_env(monkeypatch)
    check_records(run(block, lists=True)[3],
                  [("A_row/B_km", MP, HD, D, 1), ("A_row/B_km", MP, D, HD, 1), ("A_row/B_km", MP, D, D, 1), ("A_row/B_km", MP, D, 3 * D, 1)],
                  [("layernorm_bwd", M * D * 16), ("layernorm_bwd", M * D * 14), ("attention_bwd", M * D * 16)])


def test_records_full_row_kernel_forced(block, plain, monkeypatch):
    """DEVIT_GEMMFR=1 (read per call) puts the N = 384 launches on the full-row kernel and with it fuses both LayerNorm backwards into the dgrads in
    front of them: one PROFILE record each, no PROFILE_HBM record.  fc2's forward then reads the k-major copy of its weight: still "A_row/B_row"."""
    default_env(monkeypatch)
    monkeypatch.setenv("DEVIT_GEMMFR", "1")
    y, dx, _, recs = run(block, lists=True)
    check_records(recs, [("A_row/B_km", MP, HD, D, 1), ("A_row/B_km", MP, D, D, 1),
                         ("A_row/B_km+ln_bwd", MP, D, HD, 1), ("A_row/B_km+ln_bwd", MP, D, 3 * D, 1)], [("attention_bwd", M * D * 16)])
    # the kernel choice changes no bit (tests/test_gpu_fullsize.py::test_full_row_gemm_inside_the_model_full_size; fused dx: tests/test_gpu_lnfuse.py)
    assert torch.equal(y, plain[0]) and torch.equal(dx, plain[1])


def test_gradient_into_exposed_attention_output_is_refused(block):
    from devit_amd._lib import DevitError
    blk, x0 = block
    x = x0.clone().requires_grad_(True)
    att = blk(x, output_att=True)["attention"]
    with pytest.raises(DevitError, match='precision="f32"'):
        att.float().square().sum().backward()
    for p in blk.parameters():
        p.grad = None
