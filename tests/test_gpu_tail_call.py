"""The lean last block's entry points on the device, at the C-ABI level (no model): devit_token_rows_copy against indexing, bit for bit and with
everything around the addressed elements untouched; devit_tail_fwd against devit_encoder_fwd on identical inputs -- every buffer the lean block
saves on its token rows is the block's, torch.equal; and devit_tail_fwd + devit_tail_bwd audited STAGE BY STAGE on their own buffers
(tests/_block_model.py: tail_audit; tests/test_block_model.py holds that model to its planted wiring bugs without a GPU).

The audit's memory is ONE arena (K.TailArena): every buffer at exactly the size devit_tail_acts_sizes / devit_tail_bwd_sizes report, dx_in, the
caller's g2 and the accumulators behind them, a guard slot in front and behind, every byte 0x55 before the calls -- except the accumulators, whose
non-zero preload is part of the statement.  After the calls every stage holds chk(worst |err| / bound, 1.0, name="tail/<case>/<stage>") against
the float64 statement of that ONE operation on the stage's stored inputs, every pad row is zero (the caller's g2 included), x, dx and the live
rows of g2 come back bit for bit, and no byte beyond a buffer's stated extent has changed.  Every bar is 1.0 against a bound of the sibling
models, or torch.equal.  (The launch list is held in tests/test_gpu_tail_launches.py, the whole step in tests/test_gpu_lean.py.)"""
import contextlib
import ctypes as C
import os

import pytest
import torch

import _block_model as K
from _block_model import BF16, F16, F32
from conftest import chk

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
    # every buffer the backward later reads on the token rows is the block's, bit for bit
    tok = K.tok_rows(B, N, ntok, dev)
    save = bool(c["flags"] & K.SAVE)
    same = [("ln1_tok", "ln1", D, dt, slice(0, D)), ("q", "qkv", 3 * Da, dt, slice(0, Da)), ("attn_o", "attn_o", Da, dt, slice(0, Da)),
            ("x_tok", None, D, F32, slice(0, D)), ("x1", "x1", D, F32, slice(0, D)), ("ln2", "ln2", D, dt, slice(0, D)), ("h", "h", Hd, dt, slice(0, Hd))]
    same += [("h_pre", "h_pre", Hd, dt, slice(0, Hd))] if save else []
    for name, src, ld, ty, cols in same:
        want = inp["x"][tok] if src is None else blk.view(src, M, ld, ty)[tok][:, cols]
        got = tail.view(name, T, cols.stop, ty)
        assert torch.equal(bits(got), bits(want.contiguous())), (name, "token rows")
    if save:
        assert torch.equal(tail.view("mean1", 1, M, F32), blk.view("mean1", 1, M, F32))
        assert torch.equal(tail.view("rstd1", 1, M, F32), blk.view("rstd1", 1, M, F32))
        for name in ("mean2", "rstd2"):
            assert torch.equal(tail.view(name, 1, T, F32)[0], blk.view(name, 1, M, F32)[0][tok]), name
        lse_b, lse_t = blk.view("lse", B * d["H"], N, F32).view(B, d["H"], N), tail.view("lse", B * d["H"], ntok, F32).view(B, d["H"], ntok)
        assert torch.equal(lse_t, lse_b[:, :, :ntok])


# ============================================================================================ the two calls, stage by stage
@contextlib.contextmanager
def environment(env):
    """the per-call switches of the sequence: all cleared, the run's set; put back afterwards"""
    old = {k: os.environ.get(k) for k in K.ENV_SWITCHES}
    try:
        for k in K.ENV_SWITCHES:
            os.environ.pop(k, None)
        os.environ.update(env)
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


JUNK = 0x7f         # the second prefill of the transients: 3.4e38 in bf16 and in fp32, finite
BWD_SLOTS = K.TAIL_BWD_NAMES + ("dx_in", "g2")


class TailRun:
    """one case's memory -- the arena, the inputs on the device -- and the two calls"""

    def __init__(self, dev, c, env, offered):
        from devit_amd import _lib as L
        self.c, self.ntok, self.env, self.offered = c, c["ntok"], env, offered
        self.d = K.tail_dims(c, self.ntok)
        self.inp = K.to_device(K.tail_inputs(c, self.ntok), dev)
        self.x, self.dx = self.inp["x"].clone(), self.inp["dx"].clone()
        self.ar = K.tail_arena(dev, c, self.ntok)
        self.fill = {}
        self.load()
        self.jobs, self.count = (L.WgradJob * 4)(), C.c_int(-1)
        with environment(env):
            fused = bool(L.load().devit_dgrad_layernorm_bwd_fused(self.d["Tp"], self.d["D"], self.d["Hd"]))
        assert not fused, "the LN2 site of the token rows runs as two launches under the default switches: dln2 is in memory"
        self.route = K.tail_routes(c, self.ntok, env, offered, fused)

    def load(self):
        """the caller's part of the arena: the live rows of g2 (its pad rows keep the prefill: the call zeroes them), every accumulator's preload"""
        d = self.d
        self.ar.view("g2", d["Tp"], d["D"], BF16)[:d["T"]] = self.inp["g2"]
        for n, t in self.inp["acc0"].items():
            self.ar.view("g_" + n, 1, t.numel(), F32)[0] = t.reshape(-1)

    def adr(self, name):
        name = "kv" if name == "qkv" else name
        if name in self.ar.sizes:
            return self.ar.adr(name)
        t = {"x": self.x, "dx": self.dx}.get(name, self.inp["w"].get(name))
        return None if t is None else t.data_ptr()

    def structs(self):
        w, t, g, io = K.tail_structs(self.c, self.adr, self.ntok)
        io.lnws_bytes = self.ar.sizes["lnws"]
        if self.offered:
            io.defer_jobs, io.defer_count = C.addressof(self.jobs), C.addressof(self.count)
        return w, t, g, io

    def forward(self):
        from devit_amd import _lib as L
        w, t, _, _ = self.structs()
        with environment(self.env):
            L.call("devit_tail_fwd", C.byref(w), C.byref(t), self.d["B"], self.d["N"], self.d["D"], K.EPS, L.stream_ptr())

    def backward(self):
        """devit_tail_bwd, then -- as the caller of a deferred product must -- the one job through devit_wgrad_grouped over K = Mp rows"""
        from devit_amd import _lib as L
        w, t, g, io = self.structs()
        self.count.value = -1
        with environment(self.env):
            L.call("devit_tail_bwd", C.byref(w), C.byref(t), C.byref(g), C.byref(io), self.d["B"], self.d["N"], self.d["D"], K.EPS, L.stream_ptr())
            if self.offered:
                assert self.count.value == int(self.route["kv_job"]), (self.count.value, self.route)
                if self.count.value == 1:
                    L.call("devit_wgrad_grouped", self.jobs, 1, self.d["Mp"], 0, L.stream_ptr())
        torch.cuda.synchronize()

    def bufs(self):
        """the logical views tail_audit() takes, of whatever the calls left"""
        d = self.d
        out = dict(x=self.x, dx=self.dx, g2=self.ar.view("g2", d["Tp"], d["D"], BF16), dx_in=self.ar.view("dx_in", d["M"], d["D"], F32))
        for name, (rows, cols, is16) in K.tail_buffer_shapes(self.c, self.ntok).items():
            v = self.ar.view(name, rows, cols, BF16 if is16 else F32)
            out[name] = v[0] if name.startswith(("mean", "rstd")) else v
        out["acc"] = {n: self.ar.view("g_" + n, 1, t.numel(), F32)[0].view(t.shape) for n, t in self.inp["acc0"].items()}
        return out

    def audit(self):
        rt, problems = K.tail_audit(self.c, self.ntok, self.inp, self.bufs(), self.route)
        return rt, problems + self.ar.written_outside(self.fill)


_RUNS = {}


def the_run(dev, c, env, offered):
    """one forward + backward per (case, environment, slot offered), shared by the tests that need it and left unchanged"""
    key = (c["name"], tuple(sorted(env.items())), offered)
    if key not in _RUNS:
        run = TailRun(dev, c, env, offered)
        run.forward()
        run.backward()
        _RUNS[key] = run
    return _RUNS[key]


def hold_all(tag, rt, problems):
    print(f"tail/{tag}", " ".join(f"{k} {v:.3f}" for k, v in rt.items()))
    assert problems == [], f"tail/{tag}: {problems}"
    assert list(rt) == list(K.TAIL_FWD_STAGES + K.TAIL_BWD_STAGES), "no stage is left out"
    bad = [k for k, v in rt.items() if not chk(v, 1.0, name=f"tail/{tag}/{k}")]
    assert not bad, f"tail/{tag}: worst |err| / bound {({k: rt[k] for k in bad})}"


TAIL_VARIANTS = K.tail_variants()


@pytest.mark.parametrize("tag,c,env,offered", TAIL_VARIANTS, ids=[v[0] for v in TAIL_VARIANTS])
def test_tail_stages(dev, tag, c, env, offered):
    """Worst |err| / bound per stage, MI355X (profiles/tail_bwd_parity_margins.json): the 16-bit stores sit just under 1, the copies at 0 (bit for
    bit), the fp32 stages and the accumulators far below."""
    run = the_run(dev, c, env, offered)
    want = {"tail_student/split_k": -1, "tail_student/deferred": 1, "tail_student/wgradfr0": 0, "tail_one_token": 0}.get(tag, -1)
    assert run.count.value == want, "*defer_count: 1 where the all-rows product is handed out, 0 where a slot is offered and not taken"
    if want == 0:
        assert run.jobs[0].a is None and run.jobs[0].out is None, "no job written"
    hold_all(tag, *run.audit())


@pytest.mark.parametrize("c", K.TAIL_CASES, ids=[c["name"] for c in K.TAIL_CASES])
def test_tail_bwd_again_on_junk_transients(dev, c):
    """the backward a second time, on fresh accumulators, with every transient, dx_in and the pad rows of g2 prefilled with other junk: the same
    audit holds, because the call zeroes what it needs and reads nothing it has not written"""
    _, env, offered = c["runs"][0]
    run = TailRun(dev, c, env, offered)
    run.forward()
    run.backward()
    first, problems = run.audit()
    assert problems == [], problems
    run.ar.refill(BWD_SLOTS, JUNK)
    run.fill = {n: JUNK for n in BWD_SLOTS}
    run.load()
    run.backward()
    again, problems = run.audit()
    hold_all(c["name"] + "/again", again, problems)
    exact = [k for k, v in first.items() if v == 0.0]
    assert {"ln1_tok", "x_tok", "dqkv_kv", "dln1/tok"} <= set(exact) and all(again[k] == 0.0 for k in exact)


REFUSAL_CASE = K._tail_case("student", 2, 198, 2, 384, 6, 1536)      # the shape the TAIL_REFUSALS rows are worded for


@pytest.mark.parametrize("name,case,change,entry,code,words", K.TAIL_REFUSALS, ids=[r[0] for r in K.TAIL_REFUSALS])
def test_tail_entry_points_refuse(dev, name, case, change, entry, code, words):
    """the DEVIT_ERR_* with the cause in the message and nothing launched: every byte of the arena, and the inputs, come back as they were"""
    run = TailRun(dev, REFUSAL_CASE, {}, False)
    before = [run.ar.mem.clone(), run.x.clone(), run.dx.clone()]
    rc, msg = K.refused(case, change, entry, run.adr)
    assert rc == code and words in msg, (name, rc, msg)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, [run.ar.mem, run.x, run.dx])), f"{name}: a refused call wrote"
