"""The host sequence of the 16-bit encoder block -- devit_encoder_fwd / devit_block_bwd (csrc/encoder.hip) and the hand-off logic of
ops._encoder_forward_composite / _encoder_backward_composite -- on a real MI355X, audited stage by stage on its own buffers
(tests/_block_model.py; tests/test_block_model.py holds that model to its planted wiring bugs without a GPU).

The entry points are called through ctypes with test-owned memory: the buffers are carved back to back from one arena at the sizes
devit_block_acts_sizes / devit_block_bwd_sizes report, as ops.py does, with a guard band behind the last; every byte is 0xff (NaN in fp32 and in
both 16-bit types) before the call, except the gradient accumulators, whose preload is part of the statement.  After the call every stage holds
chk(worst |err| / bound, 1.0, name="block/<case>/<stage>") against the float64 statement of that ONE operation on the stage's stored inputs, every
pad row of every 16-bit buffer is zero (the qkv overhang included), and everything the call does not own -- the slack behind each buffer's
extent, the guards, the inputs -- comes back bit for bit.  Every bar is 1.0 against a bound of the sibling models, or torch.equal.

The dropped sequence (devit_encoder_fwd_drop / devit_block_bwd_drop, ops with cfg.drop) is held the same way from test_block_stages_drop on: masks
from the numpy mirror alone, the shared fp32 temporary one more guarded 0xff-filled buffer, the caller's g2 torch.equal to the masked value."""
import contextlib
import ctypes as C
import os

import pytest
import torch

import _block_model as K
from _block_model import BF16, F16, F32
from conftest import chk

pytestmark = pytest.mark.gpu
GUARD = 4096
SENT = -123.0


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from devit_amd import _lib
    _lib.require_device(torch.zeros(1, device="cuda"))
    return torch.device("cuda")


def hold(tag, r):
    assert chk(r, 1.0, name=f"block/{tag}"), f"block/{tag}: worst |err| / bound {r:.4f}"


def hold_all(tag, rt, problems):
    print(f"block/{tag}", " ".join(f"{k} {v:.3f}" for k, v in rt.items()))
    assert not problems, f"block/{tag}: {problems}"
    bad = [k for k, v in rt.items() if not chk(v, 1.0, name=f"block/{tag}/{k}")]
    assert not bad, f"block/{tag}: worst |err| / bound {({k: rt[k] for k in bad})}"


@contextlib.contextmanager
def environment(env):
    """the per-call switches of the sequence: all cleared, the variant's set; put back afterwards"""
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


class Arena:
    """buffers back to back at the given sizes, a guard band behind the last, every byte 0xff"""

    def __init__(self, dev, sizes):
        self.sizes, self.off, off = dict(sizes), {}, 0
        for name, n in sizes.items():
            assert n % 256 == 0, (name, n)
            self.off[name] = off
            off += n
        self.mem = torch.full((off + GUARD,), 0xff, dtype=torch.uint8, device=dev)
        self.end = off

    def adr(self, name):
        return self.mem.data_ptr() + self.off[name] if self.sizes[name] else None

    def view(self, name, rows, cols, dtype):
        o = self.off[name]
        return self.mem[o:o + rows * cols * dtype.itemsize].view(dtype).view(rows, cols)

    def untouched_behind(self, extents):
        """every byte between a buffer's stated extent and the next buffer, and the guard, still 0xff -> names of the buffers where not"""
        bad = [n for n, e in extents.items() if not bool((self.mem[self.off[n] + e:self.off[n] + self.sizes[n]] == 0xff).all())]
        return bad + ([] if bool((self.mem[self.end:] == 0xff).all()) else ["guard"])


class Acc:
    """a preloaded fp32 accumulator with a sentinel guard behind it"""

    def __init__(self, dev, init):
        self.n, self.shape = init.numel(), init.shape
        self.flat = torch.full((self.n + 64,), SENT, dtype=F32, device=dev)
        self.flat[:self.n] = init.reshape(-1).to(dev)

    @property
    def v(self):
        return self.flat[:self.n].view(self.shape)

    def intact(self):
        return bool((self.flat[self.n:] == SENT).all())


def check_sizes(c, acts_sz, bwd_sz):
    for got, want in ((acts_sz, K.act_extents(c)), (bwd_sz, K.bwd_extents(c))):
        for name, n in want.items():
            assert got[name] >= n and got[name] % 256 == 0 and (got[name] == 0) == (n == 0), (c["name"], name, got[name], n)


class Block:
    """one block's memory: the activation arena, the backward arena (the eight transients + dx_in + g_prev), the accumulators, the inputs on the
    device -- and the two calls"""

    def __init__(self, dev, c, inp, x=None, prev=True, own_prev_bias=True, drop=None):
        from devit_amd import _lib as L
        self.c, self.dev, self.d = c, dev, K.dims(c)
        d = self.d
        M, Mp, D = d["M"], d["Mp"], d["D"]
        self.inp = K.to_device(inp, dev)
        acts_sz, bwd_sz = K.library_sizes(c)
        check_sizes(c, acts_sz, bwd_sz)
        self.lnws = bwd_sz["lnws"]
        self.acts = Arena(dev, acts_sz)
        self.save = bool(c["flags"] & K.SAVE)
        self.t = dict(self.inp["w"])
        self.t["x"] = self.inp["x"] if x is None else x
        if self.save:
            al = lambda n: (n + 255) // 256 * 256                                               # noqa: E731
            self.bwd = Arena(dev, dict(bwd_sz, dx_in=al(M * D * 4), g_prev=al(Mp * D * 2) if prev else 0))
            g2 = torch.zeros((Mp, D), dtype=BF16, device=dev)
            g2[:M] = self.inp["g2"]
            self.t.update(dx=self.inp["dx"].clone(), g2=g2, dqkv_add=None if self.inp["dqkv_add"] is None else self.inp["dqkv_add"].clone(),
                          prev_dp2=self.inp["prev_dp2"] if prev else None)
            self.acc = {n: Acc(dev, self.inp["acc0"][n]) for n in K.ACC_NAMES + (("prev_fc2_b",) if prev and own_prev_bias else ())}
        self.prev = prev
        self.tmp = Arena(dev, dict(tmp=Mp * D * 4))      # the dropped sequence's fp32 temporary [pad_rows(M)][D]; nothing else may touch it
        self.drop, self.tmp_shared = drop, False         # tmp_shared: another block of a chain with p > 0 writes this block's temporary
        self.lib = L.load()

    def adr(self, name):
        if name == "tmp":
            return self.tmp.adr("tmp")
        if name in K.ACT_NAMES:
            return self.acts.adr(name)
        if self.save and name in self.bwd.sizes:
            return self.bwd.adr(name)
        if name.startswith("g_") and name != "g_prev":
            a = self.acc.get(name[2:]) if self.save else None
            return None if a is None else a.flat.data_ptr()
        t = self.t.get(name)
        return None if t is None else t.data_ptr()

    def structs(self):
        w, a, g, io = K.structs(self.c, self.adr)
        io.lnws_bytes = self.lnws if self.save else 0
        return w, a, g, io

    def fused_sites(self):
        d = self.d
        return (bool(self.lib.devit_dgrad_layernorm_bwd_fused(d["Mp"], d["D"], d["Hd"])),
                bool(self.lib.devit_dgrad_layernorm_bwd_fused(d["Mp"], d["D"], 3 * d["Da"])))

    def route(self, env, g2_bias_done=False):
        d = self.d
        return K.routes(self.c, env, self.lnws, self.lib.devit_colsum_workspace(d["Mp"], d["D"]), self.fused_sites(), g2_bias_done, self.prev,
                        drop=self.drop)

    def bufs(self):
        """the logical views audit() takes, of whatever the calls left"""
        dt = F16 if self.c["dtype16"] else BF16
        d = self.d
        out = dict(x=self.t["x"])
        for name, (rows, cols, is16) in K.buffer_shapes(self.c).items():
            ar = self.acts if name in K.ACT_NAMES else (self.bwd if self.save else None)
            if ar is None or not ar.sizes[name]:
                continue
            v = ar.view(name, rows, cols, (dt if name in K.ACT_NAMES else BF16) if is16 else F32)
            out[name] = v[0] if name.startswith(("mean", "rstd")) else v
        if self.save:
            out.update(dx=self.t["dx"], g2=self.t["g2"], dqkv_add=self.t["dqkv_add"], dx_in=self.bwd.view("dx_in", d["M"], d["D"], F32),
                       acc={n: a.v for n, a in self.acc.items()})
            if self.prev:
                out["g_prev"] = self.bwd.view("g_prev", d["Mp"], d["D"], BF16)
        if K.is_dropped(self.drop)[0]:
            out["tmp"] = self.tmp.view("tmp", d["Mp"], d["D"], F32)
        return out

    def untouched(self, fused=(False, False)):
        """-> what was written outside the stated extents (empty: nothing)"""
        bad = self.acts.untouched_behind(K.act_extents(self.c))
        # the temporary: only its first M rows may change, and those only under p > 0
        live = self.d["M"] * self.d["D"] * 4 if (K.is_dropped(self.drop)[0] or self.tmp_shared) else 0
        bad += ["tmp (rows >= M, or the whole of it without p > 0)" for _ in self.tmp.untouched_behind(dict(tmp=live))]
        if self.save:
            ext = dict(K.bwd_extents(self.c), dx_in=self.d["M"] * self.d["D"] * 4, g_prev=self.d["Mp"] * self.d["D"] * 2 if self.prev else 0)
            ext["lnws"] = self.bwd.sizes["lnws"]              # (scratch: whatever is inside it is the library's)
            bad += self.bwd.untouched_behind(ext)
            for i, n in enumerate(("dln2", "dln1")):          # the fused launch keeps dln on chip: the sequence zeroes the pad rows, nothing writes a live row
                if fused[i] and not bool((self.bwd.view(n, self.d["M"], self.d["D"], torch.int16) == -1).all()):
                    bad.append(n + " (live rows, fused)")
            bad += ["acc/" + n for n, a in self.acc.items() if not a.intact()]
        return bad


def run_block(dev, c, env, key=0, dqkv_add=True):
    """forward + backward of one block of a case under an environment -> (Block, route) after a synchronize"""
    from devit_amd import _lib as L
    blk = Block(dev, c, K.inputs(c, key, dqkv_add))
    w, a, g, io = blk.structs()
    with environment(env):
        route = blk.route(env) if blk.save else None
        rc, msg = K.call_fwd(1, C.byref(w), C.byref(a), c, L.stream_ptr())
        assert rc == 0, msg
        if blk.save:
            rc, msg = K.call_bwd(w, a, g, io, c, L.stream_ptr())
            assert rc == 0, msg
    torch.cuda.synchronize()
    return blk, route


_RUNS = {}


def the_run(dev, c, env):
    """one run per (case, environment), shared by the tests that need it and left unchanged"""
    key = (c["name"], tuple(sorted(env.items())))
    if key not in _RUNS:
        _RUNS[key] = run_block(dev, c, env)
    return _RUNS[key]


VARIANTS = K.variants()


@pytest.mark.parametrize("tag,c,env", VARIANTS, ids=[v[0] for v in VARIANTS])
def test_block_stages(dev, tag, c, env):
    blk, route = the_run(dev, c, env)
    bufs, dln = blk.bufs(), None
    if route is not None and any(route["fused"]):
        # the fused launch keeps dln on chip: the LayerNorm backward is audited on the dln of the two launches (the default routes), which is
        # its input to the bit where the GEMM's own input -- dh_pre, dqkv -- is the same bits in both runs
        other, oroute = the_run(dev, c, {})
        assert not any(oroute["fused"])
        dln = other.bufs()
        assert torch.equal(dln["dh_pre"], bufs["dh_pre"]) and torch.equal(dln["dqkv"], bufs["dqkv"])
    rt, problems = K.audit(c, blk.inp, bufs, route, dln)
    problems += ["written outside its extent: " + n for n in blk.untouched(route["fused"] if route else (False, False))]
    hold_all(tag, rt, problems)
    if not blk.save:          # f16: forward only; the backward refuses it, and writes nothing
        before = blk.acts.mem.clone()
        w, a, g, io = K.structs(c, lambda n: blk.adr(n) or blk.acts.mem.data_ptr())
        rc, msg = K.call_bwd(w, a, g, io, c)
        assert rc == K.ERR_ARG and "DEVIT_BLK_SAVE" in msg, (rc, msg)
        a.flags |= K.SAVE
        rc, msg = K.call_bwd(w, a, g, io, c)
        assert rc == K.ERR_ARG and "f16 blocks have no backward" in msg, (rc, msg)
        torch.cuda.synchronize()
        assert torch.equal(before, blk.acts.mem)


def test_block_stages_without_dqkv_add(dev):
    """the other variant of the inputs: no gradient arrives at qkv from outside the block"""
    c = K.case_named("student")
    blk, route = run_block(dev, c, {}, key=1, dqkv_add=False)
    rt, problems = K.audit(c, blk.inp, blk.bufs(), route)
    hold_all("student_no_add", rt, problems + blk.untouched())


@pytest.mark.parametrize("tag,name,env", [("student_fr", "student_fr", {"DEVIT_GEMMFR": "1"}), ("compacted", "compacted", {"DEVIT_GEMMFR": "1"})])
def test_fused_block_equals_unfused(dev, tag, name, env):
    c = K.case_named(name)
    got, groute = the_run(dev, c, env)
    ref, rroute = the_run(dev, c, {})
    assert groute["fused"] == (True, True), "devit_dgrad_layernorm_bwd_fused must report 1 at both sites"
    assert rroute["fused"] == (False, False)
    assert not got.untouched(groute["fused"]), "the dln2 / dln1 sentinels (and everything else outside the extents) come back untouched"
    gb, rb = got.bufs(), ref.bufs()
    for k in ("x2", "dx1", "g1", "dx_in", "g_prev", "dh_pre", "dqkv"):
        assert torch.equal(gb[k], rb[k]), k
    names = ("n2w", "n2b", "proj_b", "n1w", "n1b", "prev_fc2_b")
    rt = {n: K.ratio(g_, r_, b_) for n, g_, r_, b_ in K.backward_stages(c, got.inp, gb, groute, rb) if n in names}
    assert set(rt) == set(names)
    for n, r in rt.items():
        hold(f"{tag}/fused_vs_unfused_dln/{n}", r)


# ============================================================================================ the dropped sequence, one block
def run_block_drop(dev, c, env, drop, null_tmp=False, observe=None):
    """forward + backward of one block through devit_encoder_fwd_drop / devit_block_bwd_drop -> (Block, route) after a synchronize.  observe: a list
    that takes the name of every launch the library reports, in order"""
    from devit_amd import _lib as L, ops
    blk = Block(dev, c, K.inputs(c), drop=drop)
    w, a, g, io = blk.structs()
    dr = K.drop_struct(drop, None if null_tmp else blk.adr("tmp"))
    note = (lambda phase, stream, i: observe.append(i.name.decode()) if phase == 0 else None) if observe is not None else None
    with environment(env), (ops.observing(note) if note else contextlib.nullcontext()):
        route = blk.route(env)
        rc, msg = K.call_fwd_drop(1, C.byref(w), C.byref(a), C.byref(dr), c, L.stream_ptr())
        assert rc == 0, msg
        rc, msg = K.call_bwd_drop(w, a, g, io, dr, c, L.stream_ptr())
        assert rc == 0, msg
    torch.cuda.synchronize()
    return blk, route


def the_run_drop(dev, c, env, drop):
    key = (c["name"], tuple(sorted(env.items())), drop["p"], drop["p_attn"])
    if key not in _RUNS:
        _RUNS[key] = run_block_drop(dev, c, env, drop)
    return _RUNS[key]


DROP_VARIANTS = K.drop_variants()


@pytest.mark.parametrize("tag,c,env,drop", DROP_VARIANTS, ids=[v[0] for v in DROP_VARIANTS])
def test_block_stages_drop(dev, tag, c, env, drop):
    """Worst |err| / bound per stage, MI355X (profiles/block_drop_parity_margins.json): the 16-bit stores and x2 (two roundings, both counted) sit just
    under 1, g1 is 0 (bit for bit), the accumulators far below."""
    blk, route = the_run_drop(dev, c, env, drop)
    bufs, dln = blk.bufs(), None
    if any(route["fused"]):       # as test_block_stages: the LayerNorm backward's on-chip input from the two launches on bit-identical dh_pre / dqkv
        other, oroute = the_run_drop(dev, c, {}, drop)
        assert not any(oroute["fused"])
        dln = other.bufs()
        assert torch.equal(dln["dh_pre"], bufs["dh_pre"]) and torch.equal(dln["dqkv"], bufs["dqkv"])
    assert (route["fc2_bias"] == "masked") == (drop["p"] > 0)
    rt, problems = K.audit(c, blk.inp, bufs, route, dln, drop=drop)
    problems += ["written outside its extent: " + n for n in blk.untouched(route["fused"])]
    hold_all(tag, rt, problems)
    assert ("tmp" in rt) == (drop["p"] > 0)


ZERO_CASES = ["student", "compacted", "wide"]


@pytest.mark.parametrize("name", ZERO_CASES)
def test_zero_thresholds_are_the_plain_sequence(dev, name):
    """thr = thr_attn = 0 and tmp = NULL through the _drop entry points: the launches the plain entry points make, by name and in order; every
    forward buffer and every 16-bit or fp32 buffer of the backward to the bit; the atomically fed accumulators under their own bounds"""
    from devit_amd import ops
    c = K.case_named(name)
    zero = K.drop_of(3, 0.0, 0.0)
    plain_names, drop_names = [], []
    note = lambda phase, stream, i: plain_names.append(i.name.decode()) if phase == 0 else None      # noqa: E731
    with ops.observing(note):
        plain, proute = run_block(dev, c, {})
    got, groute = run_block_drop(dev, c, {}, zero, null_tmp=True, observe=drop_names)
    assert plain_names and drop_names == plain_names
    assert groute == proute
    assert torch.equal(got.acts.mem, plain.acts.mem), "the forward's arena, slack and guard included"
    gb, pb = got.bufs(), plain.bufs()
    for k in ("dh_pre", "dln2", "dx1", "g1", "dattn", "dqkv", "dln1", "dx_in", "g_prev", "g2", "dx"):
        assert torch.equal(gb[k], pb[k]), k
    rt, problems = K.audit(c, got.inp, gb, groute, drop=zero)
    hold_all(f"{name}/zero_thresholds", rt, problems + got.untouched(groute["fused"]))


# ============================================================================================ three blocks: driven by hand, and through ops.EncoderFn
NB = 3


def chain_inputs(c):
    """per block: its own weights, dp scales and gates (key = block index); dqkv_add on the middle block only"""
    return [K.inputs(c, key=i, dqkv_add=(i == 1)) for i in range(NB)]


_CHAINS = {}


def hand_driven_chain(dev, c):
    """(a): one devit_encoder_fwd over three blocks on separate buffers, then devit_block_bwd block by block: every block forms its own fc2 bias
    gradient (g2_bias_done = 0, no prev_fc2_b_grad), nothing deferred -> the Blocks, with their routes"""
    if c["name"] in _CHAINS:
        return _CHAINS[c["name"]]
    from devit_amd import _lib as L, ops
    d = K.dims(c)
    M, Mp, D, N = d["M"], d["Mp"], d["D"], d["N"]
    inps = chain_inputs(c)
    blks, x = [], None
    for i in range(NB):
        b = Block(dev, c, inps[i], x=x, prev=i > 0, own_prev_bias=False)
        x = b.acts.view("x2", M, D, F32)
        blks.append(b)
    st = [b.structs() for b in blks]
    ws, as_ = (L.BlockWeights * NB)(*[s[0] for s in st]), (L.BlockActs * NB)(*[s[1] for s in st])
    with environment({}):
        rc, msg = K.call_fwd(NB, ws, as_, c, L.stream_ptr())
        assert rc == 0, msg
        top = blks[-1]
        # the top block's incoming gradient: dx as given, g2 = bf16(dp2 dx) by the kernel the product path uses
        ops.call("devit_scale_cast_bf16", L.ptr(top.t["dx"]), L.ptr(top.t["g2"]), L.ptr(top.t["dp2"]), N, M, D, L.stream_ptr())
        routes = [None] * NB
        for i in range(NB - 1, -1, -1):
            b = blks[i]
            if i < NB - 1:            # the block above wrote this block's dx (its dx_in) and g2 (its g_prev)
                up = blks[i + 1]
                b.t["dx"], b.t["g2"] = up.bwd.view("dx_in", M, D, F32), up.bwd.view("g_prev", Mp, D, BF16)
            w, a, g, io = b.structs()
            io.prev_dp2 = blks[i - 1].t["dp2"].data_ptr() if i > 0 else None
            routes[i] = b.route({})
            rc, msg = K.call_bwd(w, a, g, io, c, L.stream_ptr())
            assert rc == 0, msg
    torch.cuda.synchronize()
    for i, b in enumerate(blks):      # what the audit states the stages on: the dx / g2 / dp scale each block was really given
        b.inp = dict(b.inp, x=None, dx=None, g2=None, prev_dp2=blks[i - 1].t["dp2"] if i > 0 else None)
    _CHAINS[c["name"]] = (blks, routes, inps)
    return _CHAINS[c["name"]]


@pytest.mark.parametrize("name", ["student", "wide"])
def test_three_block_chain_by_hand(dev, name):
    c = K.case_named(name)
    blks, routes, _ = hand_driven_chain(dev, c)
    for i, b in enumerate(blks):
        rt, problems = K.audit(c, b.inp, b.bufs(), routes[i])
        hold_all(f"chain_{name}/block{i}", rt, problems + b.untouched())


def encoder_fn_chain(dev, c, inps, policy, rates=None, denc=None, want_att=False):
    """(b): the same three blocks through ops.EncoderFn -> (x2 per block, qkv per block, gradient into x, {block: {accumulator: tensor}}).  rates:
    [(p, p_attn)] per block -> cfg.drop at K.DROP_SEED.  denc: a gradient that arrives for the MIDDLE block's exposed output"""
    from devit_amd import ops
    d = K.dims(c)
    M, B, N, D, Da = d["M"], d["B"], d["N"], d["D"], d["Da"]
    bps, flat, dps = [], [], []
    for inp in inps:
        w = K.to_device(inp["w"], dev)
        bp = ops.BlockParams()
        for n in ("n1w", "n1b", "qkv_b", "proj_b", "n2w", "n2b", "fc1_b", "fc2_b"):
            setattr(bp, n, w[n].clone().requires_grad_(True))
        for n in ("qkv_w", "proj_w", "fc1_w", "fc2_w"):
            setattr(bp, n + "16", w[n + "16"])
            setattr(bp, n, w[n + "16"].float().requires_grad_(True))
        bp.fc2_w16t, bp.num_heads, bp.head_gate, bp.neuron_gate = None, d["H"], w["head_gate"], w["neuron_gate"]
        bp.dp_prob, bp.module, bp.compacted, bp.masters, bp.finish = 0.0, None, False, None, None
        for n in K.ACC_NAMES:
            getattr(bp, n).grad = inp["acc0"][n].to(dev).clone()
        dps.append((w["dp1"], w["dp2"]))
        bps.append(bp)
        flat += bp.all_params()
    cfg = ops.EncoderCfg(bps, True, dps, True, want_att, True)
    cfg.grad_enabled = True
    if rates is not None:
        cfg.drop = (K.DROP_SEED, list(rates))
    x = inps[0]["x"].to(dev).view(B, N, D).clone().requires_grad_(True)
    with environment({"DEVIT_WGRAD_GROUP": policy}):
        outs = ops.EncoderFn.apply(x, cfg, *flat)
        xo, qkvs, encs = outs[0], outs[1:1 + NB], outs[1 + NB:]
        add = torch.zeros_like(qkvs[1])
        add[:M] = inps[1]["dqkv_add"].to(dev)
        heads, grads_in = [xo, qkvs[1]], [inps[NB - 1]["dx"].to(dev).view(B, N, D), add]
        if denc is not None:
            heads, grads_in = heads + [encs[1]], grads_in + [denc.to(dev).view(B, N, D)]
        torch.autograd.backward(heads, grads_in)
    torch.cuda.synchronize()
    grads = [{n: getattr(bp, n).grad for n in K.ACC_NAMES} for bp in bps]
    return [e.detach().reshape(M, D) for e in encs], [q.detach()[:M] for q in qkvs], x.grad.reshape(M, D), grads


BIAS_AND_WEIGHTS = set(K.ACC_NAMES)


@pytest.mark.parametrize("policy", ["all", "block"])
@pytest.mark.parametrize("name", ["student", "wide"])
def test_three_block_chain(dev, name, policy):
    """the hand-off logic of ops.py -- fc2's bias gradient handed down by the block above, the deferred weight-gradient groups, the two g slots and
    the two alternating dx buffers -- against the hand-driven chain: activations and the gradient into the encoder input to the bit, every
    parameter gradient under the float64 reference and bound computed from the hand-driven chain's stored buffers"""
    from _tail_model import ln_colsum_bounds
    c = K.case_named(name)
    blks, routes, inps = hand_driven_chain(dev, c)
    x2s, qkvs, dx_in, grads = encoder_fn_chain(dev, c, inps, policy)
    M = K.dims(c)["M"]
    for i, b in enumerate(blks):
        ab = b.bufs()
        assert torch.equal(x2s[i], ab["x2"]), f"x2 of block {i}"
        assert torch.equal(qkvs[i], ab["qkv"][:M]), f"qkv of block {i}"
    assert torch.equal(dx_in, blks[0].bufs()["dx_in"]), "the gradient into the encoder input"
    for i, b in enumerate(blks):
        ab = b.bufs()
        handed = i < NB - 1                  # every block but the topmost gets fc2's bias gradient from the LayerNorm backward of the block above
        route = dict(routes[i], fc2_bias="handed") if handed else routes[i]
        rt = {n: K.ratio(grads[i][n], r_, b_) for n, _, r_, b_ in K.backward_stages(c, b.inp, ab, route) if n in BIAS_AND_WEIGHTS and not (handed and n == "fc2_b")}
        if handed:
            ref, bnd = ln_colsum_bounds(ab["g2"][:M], b.inp["acc0"]["fc2_b"])
            rt["fc2_b"] = K.ratio(grads[i]["fc2_b"], ref, bnd)
        assert set(rt) == BIAS_AND_WEIGHTS
        print(f"block/chain_{name}_{policy}/block{i}", " ".join(f"{k} {v:.3f}" for k, v in rt.items()))
        for n, r in rt.items():
            hold(f"chain_{name}_{policy}/block{i}/{n}", r)


# ============================================================================================ three blocks with MIXED dropout rates
RATE_ORDERS = {"mixed": [(0.1, 0.0), (0.0, 0.1), (0.1, 0.1)], "middle": [(0.0, 0.0), (0.1, 0.1), (0.0, 0.0)]}


def chain_denc(c):
    d = K.dims(c)
    return 0.5 * K.T.randn(K.gen("block", c["name"], "denc"), d["M"], d["D"])


def hand_driven_chain_drop(dev, c, order, inject):
    """One devit_encoder_fwd_drop over three blocks that share ONE temporary, then devit_block_bwd_drop block by block as the header states the
    hand-off: g2_bias_done = 0 and no prev_fc2_b_grad anywhere (every block forms its own fc2 bias gradient; a block with p > 0 must).  What a later
    call rewrites in place is kept as it was when its stage was written: a block's g_prev before the block below masks it (site 4) and, with
    `inject`, the top block's dx_in / g_prev before devit_add_scale_cast_bf16 adds the middle block's exposed-output gradient.
    -> (Blocks, routes, inputs, dropout descriptions)"""
    key = (c["name"], order, inject)
    if key in _CHAINS:
        return _CHAINS[key]
    from devit_amd import _lib as L, ops
    d = K.dims(c)
    M, Mp, D, N = d["M"], d["Mp"], d["D"], d["N"]
    inps = chain_inputs(c)
    drops = [K.drop_of(i, *RATE_ORDERS[order][i]) for i in range(NB)]
    blks, x = [], None
    for i in range(NB):
        b = Block(dev, c, inps[i], x=x, prev=i > 0, own_prev_bias=False, drop=drops[i])
        x = b.acts.view("x2", M, D, F32)
        blks.append(b)
    tmp = blks[0].adr("tmp")
    blks[0].tmp_shared = True
    st = [b.structs() for b in blks]
    ws, as_ = (L.BlockWeights * NB)(*[s[0] for s in st]), (L.BlockActs * NB)(*[s[1] for s in st])
    drs = (L.BlockDropout * NB)(*[K.drop_struct(dr, tmp) for dr in drops])
    with environment({}):
        rc, msg = K.call_fwd_drop(NB, ws, as_, drs, c, L.stream_ptr())
        assert rc == 0, msg
        top = blks[-1]
        ops.call("devit_scale_cast_bf16", L.ptr(top.t["dx"]), L.ptr(top.t["g2"]), L.ptr(top.t["dp2"]), N, M, D, L.stream_ptr())
        routes = [None] * NB
        for i in range(NB - 1, -1, -1):
            b = blks[i]
            b.kept = {}
            if i < NB - 1:            # the block above wrote this block's dx (its dx_in) and g2 (its g_prev)
                up = blks[i + 1]
                b.t["dx"], b.t["g2"] = up.bwd.view("dx_in", M, D, F32), up.bwd.view("g_prev", Mp, D, BF16)
                up.kept = dict(dx_in=b.t["dx"].clone(), g_prev=b.t["g2"].clone())
                if inject and i == 1:
                    add = chain_denc(c).to(dev)
                    ops.call("devit_add_scale_cast_bf16", L.ptr(b.t["dx"]), L.ptr(add), L.ptr(b.t["g2"]), L.ptr(b.t["dp2"]), N, M, D, L.stream_ptr())
            b.g2_given = b.t["g2"][:M].clone()
            w, a, g, io = b.structs()
            io.prev_dp2 = blks[i - 1].t["dp2"].data_ptr() if i > 0 else None
            routes[i] = b.route({})
            rc, msg = K.call_bwd_drop(w, a, g, io, drs[i], c, L.stream_ptr())
            assert rc == 0, msg
    torch.cuda.synchronize()
    for i, b in enumerate(blks):      # what the audit states the stages on: the dx / g2 / dp scale each block was really given
        b.inp = dict(b.inp, x=None, dx=None, g2=b.g2_given, prev_dp2=blks[i - 1].t["dp2"] if i > 0 else None)
    _CHAINS[key] = (blks, routes, inps, drops)
    return _CHAINS[key]


def chain_bufs(blks, i):
    """block i's buffers as its own call left them, with the tmp stage only where the shared temporary still holds this block's fc2 output"""
    ab = dict(blks[i].bufs(), **blks[i].kept)
    if "tmp" in ab:
        ab["tmp"] = blks[0].tmp.view("tmp", *ab["tmp"].shape, F32)       # the ONE temporary of the call: block 0's
    if any(K.is_dropped(b.drop)[0] for b in blks[i + 1:]):
        ab.pop("tmp", None)
    return ab


DROP_CHAINS = [("student_drop", "mixed", False), ("student_drop", "middle", False), ("wide_drop", "mixed", False), ("wide_drop", "middle", False),
               ("student_drop", "mixed", True), ("wide_drop", "middle", True)]


@pytest.mark.parametrize("name,order,inject", DROP_CHAINS, ids=[f"{n}-{o}" + ("-inject" if j else "") for n, o, j in DROP_CHAINS])
def test_three_block_chain_drop_by_hand(dev, name, order, inject):
    c = K.case_named(name)
    blks, routes, _, drops = hand_driven_chain_drop(dev, c, order, inject)
    for i, b in enumerate(blks):
        rt, problems = K.audit(c, b.inp, chain_bufs(blks, i), routes[i], drop=drops[i])
        hold_all(f"chain_{name}_{order}{'_inject' if inject else ''}/block{i}", rt, problems + b.untouched())


@pytest.mark.parametrize("policy", ["all", "block"])
@pytest.mark.parametrize("name,order,inject", DROP_CHAINS, ids=[f"{n}-{o}" + ("-inject" if j else "") for n, o, j in DROP_CHAINS])
def test_three_block_chain_drop(dev, name, order, inject, policy):
    """ops._encoder_forward_composite / _drop_structs / _encoder_backward_composite under cfg.drop with per-block rates against the hand-driven chain:
    activations and the gradient into the encoder input to the bit; every parameter gradient under the reference and bound of the hand-driven
    chain's stored buffers; every block's fc2 bias gradient with exactly ONE owner -- its own masked g2 (p > 0), else the LayerNorm backward of the
    block above (`handed`), else (the top block, or a block whose incoming gradient got an exposed-output term: injected()) its own column sums"""
    from _tail_model import ln_colsum_bounds
    c = K.case_named(name)
    blks, routes, inps, drops = hand_driven_chain_drop(dev, c, order, inject)
    x2s, qkvs, dx_in, grads = encoder_fn_chain(dev, c, inps, policy, rates=RATE_ORDERS[order], denc=chain_denc(c) if inject else None)
    M = K.dims(c)["M"]
    for i, b in enumerate(blks):
        ab = b.bufs()
        assert torch.equal(x2s[i], ab["x2"]), f"x2 of block {i}"
        assert torch.equal(qkvs[i], ab["qkv"][:M]), f"qkv of block {i}"
    assert torch.equal(dx_in, blks[0].bufs()["dx_in"]), "the gradient into the encoder input"
    owners = []
    for i, b in enumerate(blks):
        ab = chain_bufs(blks, i)
        masked = drops[i]["p"] > 0
        handed = not masked and i < NB - 1 and not (inject and i == 1)
        owners.append("masked" if masked else "handed" if handed else routes[i]["fc2_bias"])
        route = dict(routes[i], fc2_bias="handed") if handed else routes[i]
        rt = {n: K.ratio(grads[i][n], r_, b_) for n, _, r_, b_ in K.backward_stages(c, b.inp, ab, route, drop=drops[i])
              if n in BIAS_AND_WEIGHTS and not (handed and n == "fc2_b")}
        g2 = ab["g2"][:M]             # as block i's call left it: masked where p > 0, as given where not
        if handed:
            ref, bnd = ln_colsum_bounds(g2, b.inp["acc0"]["fc2_b"])
            rt["fc2_b"] = K.ratio(grads[i]["fc2_b"], ref, bnd)
        assert set(rt) == BIAS_AND_WEIGHTS
        twice = grads[i]["fc2_b"].double() - (b.inp["acc0"]["fc2_b"].double() + 2 * g2.double().sum(0))
        assert float(twice.abs().max()) > 1.0, "the inputs tell one owner from two"
        print(f"block/chain_{name}_{order}{'_inject' if inject else ''}_{policy}/block{i}", owners[-1], " ".join(f"{k} {v:.3f}" for k, v in rt.items()))
        for n, r in rt.items():
            hold(f"chain_{name}_{order}{'_inject' if inject else ''}_{policy}/block{i}/{n}", r)
    want = {("mixed", False): ["masked", "handed", "masked"], ("middle", False): ["handed", "masked", None],
            ("mixed", True): ["masked", None, "masked"], ("middle", True): ["handed", "masked", None]}[(order, inject)]
    assert all(w_ is None or w_ == o for w_, o in zip(want, owners)), owners


def test_want_att_under_dropout_raises_before_any_launch(dev):
    from devit_amd import _lib as L, ops
    c = K.case_named("student_drop")
    seen = []
    with ops.observing(lambda phase, stream, i: seen.append(i.name.decode())):
        with pytest.raises(L.DevitError, match="output_att under dropout"):
            encoder_fn_chain(dev, c, chain_inputs(c), "all", rates=RATE_ORDERS["mixed"], want_att=True)
    assert not seen, seen


# ============================================================================================ refusals
@pytest.mark.parametrize("name,case,change,entry,code,words", K.REFUSALS, ids=[r[0] for r in K.REFUSALS])
def test_block_entry_points_refuse(dev, name, case, change, entry, code, words):
    """the DEVIT_ERR_* with the cause in the message, nothing launched: every buffer comes back bit for bit"""
    c = K.case_named(case)
    cc = c if c["flags"] & K.SAVE else dict(c, flags=c["flags"] | K.SAVE, dtype16=0)      # (memory for the backward's buffers too)
    blk = Block(dev, cc, K.inputs(cc))
    before = [blk.acts.mem.clone(), blk.bwd.mem.clone(), blk.tmp.mem.clone(), blk.t["g2"].clone()] + [a.flat.clone() for a in blk.acc.values()]
    rc, msg = K.refused(case, change, entry, lambda n: blk.adr(n))
    assert rc == code and words in msg, (name, rc, msg)
    torch.cuda.synchronize()
    after = [blk.acts.mem, blk.bwd.mem, blk.tmp.mem, blk.t["g2"]] + [a.flat for a in blk.acc.values()]
    assert all(torch.equal(x, y) for x, y in zip(before, after)), f"{name}: a refused call wrote"


def test_sizes_functions_refuse_on_the_device(dev):
    for name, rc, msg, code, words in K.sizes_refusals():
        assert rc == code and words in msg, (name, rc, msg)
