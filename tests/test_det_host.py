"""Deterministic mode, the host side (no GPU): the process-wide switch of the library (devit_set / get_deterministic, DEVIT_DETERMINISTIC), its
mirror in devit_amd.ops (set_deterministic, is_deterministic, the context manager), the --deterministic flag of the three training scripts, and the
refusal of a launch whose partial sums have no workspace to go to (devit_gemm_route: the argument checks of devit_gemm_bf16, nothing launched)."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def ops():
    from devit_amd import ops
    before = ops.is_deterministic()
    yield ops
    ops.set_deterministic(before)


def _child(code, **env):
    e = {k: v for k, v in os.environ.items() if k != "DEVIT_DETERMINISTIC"}
    e.update(env)
    e["PYTHONPATH"] = ROOT + os.pathsep + e.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, "-c", code], env=e, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return r.stdout.strip()


ASK = "from devit_amd import ops, _lib as L; print(int(ops.is_deterministic()), L.load().devit_get_deterministic())"


def test_default_is_off():
    assert _child(ASK) == "0 0"


def test_environment_variable_turns_it_on():
    assert _child(ASK, DEVIT_DETERMINISTIC="1") == "1 1"
    assert _child(ASK, DEVIT_DETERMINISTIC="0") == "0 0"


def test_setter_getter_round_trip(ops):
    from devit_amd import _lib as L
    lib = L.load()
    for flag in (True, False, True, False):
        ops.set_deterministic(flag)
        assert ops.is_deterministic() is flag and lib.devit_get_deterministic() == int(flag)
    assert lib.devit_set_deterministic(2) == -2 and b"neither 0 nor 1" in lib.devit_last_error()
    assert ops.is_deterministic() is False


def test_context_manager_restores(ops):
    ops.set_deterministic(False)
    with ops.deterministic():
        assert ops.is_deterministic()
        with ops.deterministic(False):
            assert not ops.is_deterministic()
        assert ops.is_deterministic()
    assert not ops.is_deterministic()
    with pytest.raises(ZeroDivisionError):
        with ops.deterministic():
            assert ops.is_deterministic()
            1 / 0
    assert not ops.is_deterministic()
    ops.set_deterministic(True)
    with ops.deterministic():
        pass
    assert ops.is_deterministic()


def test_abi_version_of_library_and_binding():
    """(the mode added symbols without a new version, 3; 4 came with the lean last block's entry points)"""
    from devit_amd import _lib as L
    assert L.load().devit_version() == 4 and L.ABI_VERSION == 4


def test_workspace_bound_needs_no_device():
    from devit_amd import _lib as L
    assert L.load().devit_det_workspace_bytes() >= 247 * (256 * 384 + 256) * 4          # one block's 19 tiles in 13 slices


@pytest.mark.parametrize("script", ["distill_sub", "train_subdata", "ensemble"])
def test_parsers_accept_the_flag(script):
    sys.path.insert(0, ROOT)
    try:
        mod = __import__(script)
    finally:
        sys.path.remove(ROOT)
    p = mod.get_args_parser()
    assert p.parse_args([]).deterministic is False
    assert p.parse_args(["--deterministic"]).deterministic is True


def test_a_launch_without_workspace_is_refused(ops):
    """A split-K ATOMIC_F32 launch in deterministic mode with nothing registered: DEVIT_ERR_ARG and a message that names the bytes; the same launch
    description with the mode off, and a one-slice launch without row sums (one partial per address: the default kernel) in the mode, pass."""
    from devit_amd import _lib as L
    lib = L.load()
    assert lib.devit_set_det_workspace(None, 0) == 0
    a, b, out, aux = 0x100000, 0x200000, 0x300000, 0x400000
    kw = dict(kind=L.EPI_ATOMIC_F32, out=out, ldc=128)
    ops.set_deterministic(True)
    L.before_call = None       # (on a GPU machine ops would register the device's workspace before the query: this test is about its absence)
    assert ops.gemm_route(a, 128, 1, b, 128, 1, 128, 128, 768, split_k=3, **kw) == -2
    msg = lib.devit_last_error().decode()
    assert "deterministic mode needs %d bytes" % (3 * 128 * 128 * 4) in msg and "devit_set_det_workspace" in msg
    assert ops.gemm_route(a, 128, 1, b, 128, 1, 128, 128, 768, split_k=1, **kw) == L.ROUTE_TILE128
    assert ops.gemm_route(a, 128, 1, b, 256, 1, 128, 256, 768, split_k=1, aux=aux, **dict(kw, ldc=256)) == -2      # row sums: one partial per n-tile
    # a registered workspace that is too small is refused the same way; one that is large enough is not (no pointer is dereferenced here)
    assert lib.devit_set_det_workspace(0x500000, 3 * 128 * 128 * 4 - 4) == 0
    assert ops.gemm_route(a, 128, 1, b, 128, 1, 128, 128, 768, split_k=3, **kw) == -2
    assert lib.devit_set_det_workspace(0x500000, 3 * 128 * 128 * 4) == 0
    assert ops.gemm_route(a, 128, 1, b, 128, 1, 128, 128, 768, split_k=3, **kw) == L.ROUTE_TILE128
    assert lib.devit_set_det_workspace(0x500004, 64) == -2
    # batched ATOMIC_F32 launches whose outputs overlap would add into one address in arrival order: refused in the mode, whatever the slice count
    for sk in (1, 3):
        assert ops.gemm_route(a, 128, 1, b, 128, 1, 128, 128, 768, split_k=sk, batch=2, a_bs=768 * 128, b_bs=768 * 128, out_bs=0, **kw) == -2
        assert "outputs overlap" in lib.devit_last_error().decode()
    assert lib.devit_set_det_workspace(0x500000, 2 * 3 * 128 * 128 * 4) == 0
    assert ops.gemm_route(a, 128, 1, b, 128, 1, 128, 128, 768, split_k=3, batch=2, a_bs=768 * 128, b_bs=768 * 128, out_bs=128 * 128, **kw) == L.ROUTE_TILE128
    assert lib.devit_set_det_workspace(None, 0) == 0
    ops._det_ws.clear()        # (on a GPU machine: the next launch in the mode registers a workspace again)
    ops.set_deterministic(False)
    assert ops.gemm_route(a, 128, 1, b, 128, 1, 128, 128, 768, split_k=3, **kw) == L.ROUTE_TILE128
