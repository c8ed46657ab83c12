"""The lean last block's entry points on the device, at the C-ABI level (no model): devit_token_rows_copy against indexing, bit for bit and with
everything around the addressed elements untouched, and devit_tail_fwd against devit_encoder_fwd on identical inputs -- the token rows of the
block's output are the lean block's output, torch.equal.  (The backward is held through the model: tests/test_gpu_lean.py, and launch for launch
in tests/test_gpu_tail_launches.py.)"""
import ctypes as C

import pytest
import torch

import _block_model as K
from _block_model import BF16, F16, F32

pytestmark = pytest.mark.gpu
GUARD = 16          # sentinel rows in front of and behind every matrix


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda")


def bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def matrix(g, rows, ld, dtype):
    """[GUARD + rows + GUARD][ld] of random values: whatever the copy does not address is a sentinel of its own"""
    return (torch.randn((rows + 2 * GUARD, ld), generator=g) * 3).to(dtype)


# (dtype, B, rows per image of the source / of the destination, ntok, cols, source ld, destination ld, destination column offset, add)
COPIES = {
    "gather_bf16_one_token": (BF16, 3, 5, 1, 1, 128, 128, 128, 0, 0),
    "scatter_bf16_one_token": (BF16, 3, 1, 5, 1, 128, 128, 128, 0, 0),
    "bf16_into_a_column_block": (BF16, 2, 198, 2, 2, 768, 768, 1152, 384, 0),
    "add_f32_onto_token_rows": (F32, 3, 2, 51, 2, 384, 384, 384, 0, 1),
}


@pytest.mark.parametrize("name", list(COPIES))
def test_token_rows_copy(dev, name):
    from devit_amd import _lib as L
    dtype, B, src_rpi, dst_rpi, ntok, cols, src_ld, dst_ld, c0, add = COPIES[name]
    g = torch.Generator().manual_seed(len(name))
    src, dst = matrix(g, B * src_rpi, src_ld, dtype), matrix(g, B * dst_rpi, dst_ld, dtype)
    want = dst.clone()
    sv = src[GUARD:GUARD + B * src_rpi].view(B, src_rpi, src_ld)[:, :ntok, :cols]
    wv = want[GUARD:GUARD + B * dst_rpi].view(B, dst_rpi, dst_ld)[:, :ntok, c0:c0 + cols]
    wv.copy_(wv + sv if add else sv)                  # (one fp32 addition per element: the same bits on any machine)
    s, d = src.to(dev), dst.to(dev)
    e = s.element_size()
    L.call("devit_token_rows_copy", C.c_void_p(s.data_ptr() + GUARD * src_ld * e), src_rpi, src_ld,
           C.c_void_p(d.data_ptr() + (GUARD * dst_ld + c0) * e), dst_rpi, dst_ld, B, ntok, cols, e, add, L.stream_ptr())
    torch.cuda.synchronize()
    assert torch.equal(bits(d.cpu()), bits(want)), name
    assert torch.equal(bits(s.cpu()), bits(src)), "the source is read only"


# (name, B, N, D, heads, hidden, flags, dtype16), ntok
TAIL_CASES = [
    (K._case("tail_small", 2, 5, 128, 2, 128, K.SAVE), 1),
    (K._case("tail_student", 3, 198, 384, 6, 1536, K.SAVE), 2),          # head and neuron gates, DropPath scales: K.block_weights
    (K._case("tail_f16", 3, 51, 256, 4, 512, 0, dtype16=1), 2),          # the frozen teacher's type: forward only
]


class Arena:
    """one allocation for the buffers of a sizes function, filled with 0x55 bytes (pad rows must come out zero)"""

    def __init__(self, dev, sizes, names):
        self.offs, off = {}, 0
        for n, s in zip(names, sizes):
            self.offs[n] = (off, s)
            off += s
        self.mem = torch.full((off,), 0x55, dtype=torch.uint8, device=dev)

    def adr(self, name):
        off, s = self.offs[name]
        return self.mem.data_ptr() + off if s else None

    def view(self, name, rows, cols, dtype):
        off = self.offs[name][0]
        return self.mem[off:off + rows * cols * dtype.itemsize].view(dtype).view(rows, cols)


TAIL_NAMES = K.ACT_NAMES + ("ln1_tok", "q", "x_tok")


@pytest.mark.parametrize("c,ntok", TAIL_CASES, ids=[c["name"] for c, _ in TAIL_CASES])
def test_tail_fwd_equals_the_token_rows_of_the_block(dev, c, ntok):
    from devit_amd import _lib as L
    d = K.dims(c)
    B, N, D, Da, Hd, M = d["B"], d["N"], d["D"], d["Da"], d["Hd"], d["M"]
    T, Tp = B * ntok, K.pad_rows(B * ntok)
    dt = F16 if c["dtype16"] else BF16
    inp = K.to_device(K.inputs(c, dqkv_add=False), dev)
    w = inp["w"]

    def adr_in(arena):
        def adr(name):
            if name in arena.offs:
                return arena.adr(name)
            t = inp["x"] if name == "x" else w.get(name)
            return None if t is None else t.data_ptr()
        return adr
    sa, st = (C.c_size_t * L.ACT_COUNT)(), (C.c_size_t * L.TAIL_ACT_COUNT)()
    L.call("devit_block_acts_sizes", B, N, D, Da, Hd, c["flags"], sa)
    L.call("devit_tail_acts_sizes", B, N, ntok, D, Da, Hd, c["flags"], st)
    blk, tail = Arena(dev, sa, K.ACT_NAMES), Arena(dev, st, TAIL_NAMES)
    ws, a_blk, _, _ = K.structs(c, adr_in(blk))
    rc, msg = K.call_fwd(1, C.byref(ws), C.byref(a_blk), c, L.stream_ptr())
    assert rc == 0, msg
    t = L.TailActs()
    t.acts = K.structs(c, adr_in(tail))[1]
    t.ln1_tok, t.q, t.x_tok, t.ntok = tail.adr("ln1_tok"), tail.adr("q"), tail.adr("x_tok"), ntok
    L.call("devit_tail_fwd", C.byref(ws), C.byref(t), B, N, D, K.EPS, L.stream_ptr())
    torch.cuda.synchronize()
    x2 = blk.view("x2", M, D, F32).view(B, N, D)
    assert torch.equal(tail.view("x2", T, D, F32).view(B, ntok, D), x2[:, :ntok])
    assert bool(torch.isfinite(x2).all())
    # what the two sequences share on all rows, and the pad rows the call zeroes
    assert torch.equal(bits(tail.view("ln1", d["Mp"], D, dt)), bits(blk.view("ln1", d["Mp"], D, dt)))
    assert torch.equal(bits(tail.view("qkv", d["Mp"], 2 * Da, dt)), bits(blk.view("qkv", d["Mp"], 3 * Da, dt)[:, Da:]))
    for name, cols in (("ln1_tok", D), ("q", Da), ("attn_o", Da), ("ln2", D), ("h", Hd)) + ((("h_pre", Hd),) if c["flags"] & K.SAVE else ()):
        assert not bool(bits(tail.view(name, Tp, cols, dt))[T:].any()), (name, "pad rows")
    if c["flags"] & K.SAVE:
        assert torch.equal(tail.view("mean1", 1, M, F32), blk.view("mean1", 1, M, F32))
        lse_b, lse_t = blk.view("lse", B * d["H"], N, F32).view(B, d["H"], N), tail.view("lse", B * d["H"], ntok, F32).view(B, d["H"], ntok)
        assert torch.equal(lse_t, lse_b[:, :, :ntok])
