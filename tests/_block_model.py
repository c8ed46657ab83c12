"""The host sequence of the 16-bit encoder block (csrc/encoder.hip: devit_encoder_fwd, devit_block_bwd) audited STAGE BY STAGE: every buffer a block
leaves in memory is compared with the float64 statement of the ONE operation that produced it, evaluated on that operation's inputs exactly as
they were left in memory, under the per-element bound the project already holds that kernel to:
    LayerNorm forward / backward and their column sums   _tail_model.ln_fwd_bounds, ln_bwd_bounds, ln_colsum_bounds
    the GEMM launches                                    _gemm_model.statement (per epilogue kind), wgrad_reference (the grouped weight gradients)
    attention forward / backward                         _attn_model.bounds
A wrong wire -- another buffer, flag, row scale or bias pointer, a pad row left with junk, a bias gradient counted twice -- is an error of the size
of the signal on ONE named stage; no tolerance is made up for the composition (whose end-to-end accuracy stays with tests/test_gpu_model.py).
Plain torch: everything runs where its inputs live.  Shared by tests/test_block_model.py (this model under test, no GPU: emulate() and its
planted wiring bugs) and tests/test_gpu_block.py (the sequence under test).

Two bounds are not in the sibling models and are counted here by their convention (u per rounding on the sum of the absolute terms):
    g = bf16(rowscale * dx) of the LayerNorm backward (ln_rows.h: one fp32 product, one rounding to bf16): stored16(u |ref|, ref); the project's
        own test of that kernel (tests/test_gpu_tail.py) holds it to the same bits as torch's product of the RETURNED dx, which is stricter
    devit_colsum_bf16 (elementwise.hip: colsum_bf16_kernel + sum_partials_kernel) on non-integer data: colsum_pass_roundings() below.

Cases (B, N, D, heads, hidden): the smallest shapes at which each branch of the sequence is taken; every M = B N is off the 256-row grid.
    student     2 x 198, 384 / 6 / 1536   default routes: grouped weight gradients (D == 384), the column-sum pass for fc2's bias, QKV_PAD (128), ATT
    student_fr  the same under DEVIT_GEMMFR=1 with fc2_w16t: fc2 forward on the k-major copy, both dgrad + LayerNorm sites fused
    compacted   3 x 51, 384 / 4 (attn_width 256) / 640: qkv_pad_rows = 205, one row tile; default, DEVIT_GEMMFR=1, DEVIT_WGRADFR=0.  Its LayerNorm
                workspace (20 workgroups) is smaller than the column-sum pass needs, so fc2's bias gradient comes from fc2's own split-K launch
    wide        2 x 197, 256 / 4 / 512: wmode == 0, four split-K launches on the side stream (and on the caller's with DEVIT_WGRAD_STREAM=0)
    short       4 x 17, 384 / 6 / 768: many images per tile
    f16_fwd     1 x 208, 256 / 4 / 512, f16, no DEVIT_BLK_SAVE: forward only (one image: dp1 and dp2 are single values, 1.25 and 0.5)
(devit_gemm_bf16 accepts every product of these shapes: none had to be moved.)

The dropped sequence (devit_encoder_fwd_drop / devit_block_bwd_drop) is the same audit with a per-block description (drop_of(): seed, block index,
p, p_attn).  thr / s come from _drop_model.thr_s and every mask from the numpy mirror (tests/_philox.py through _drop_model._keep and
_attn_model.attn_keep), never from devit_dropout_mask.  No bound is new: the attention stages take _attn_model.bounds(..., keep, s); `tmp` is fc2's
STORE_F32 statement; x2 _drop_model.residual_statement with judge_residual's bound; fc2_b / proj_b the column sums of the masked g2 / g1 under
apply_statement's bound.  Where a pass rewrites or loses a stage's buffer two statements compose (x1: residual_stage(e_y); h, dh_pre:
masked_in_place()); g1 and the caller's g2 are held bit for bit.  DROP_CASES (no DEVIT_BLK_ATT: refused under p > 0), rates (p, p_attn):
    student_drop     2 x 198, 384 / 6 / 1536, block 5, (0.1, 0.1): grouped weight gradients, NO column-sum pass for fc2's bias, ceil4(198) = 200
    student_fr_drop  the same under DEVIT_GEMMFR=1 with fc2_w16t, block 0, (0.5, 0): both fused sites with a NULL column-sum pointer, fc2_w16t not taken
    compacted_drop   3 x 51, 384 / 4 / 640, block 11; default and DEVIT_WGRADFR=0; (0, 0.25): attention-only dropout on the plain sequence,
                     ceil4(51) = 52, and (0.1, 0.1)
    wide_drop        2 x 197, 256 / 4 / 512, block 5, (0.1, 0.1): split-K weight gradients on the side stream (and DEVIT_WGRAD_STREAM=0) reading
                     buffers masked in place on the caller's stream

The lean last block (devit_tail_fwd / devit_tail_bwd) is audited the same way at the end of this file: tail_forward_stages / tail_backward_stages /
tail_audit / tail_emulate and TAIL_MUTATIONS.  Its branch half is the block's own code on the T = B ntok token rows, so both audits -- and both
emulations -- call the same statements: branch_forward_stages / branch_backward_stages (_emu_branch_fwd / _emu_branch_bwd) take (rows, padded rows,
rows per DropPath scale).  One bound is counted there: the token rows of dx_in, where a separate pass adds the stored fp32 dx1 to the stored fp32
LayerNorm backward -- one fp32 rounding of the sum, U |reference| by the convention above, on top of ln_bwd_bounds without a residual.
TAIL_CASES (B, N, ntok, D, heads, hidden), every M and T off the 256-row grid:
    tail_student      3 x 198, 2, 384 / 6 / 1536: the all-rows product split-K; handed out as a job; offered a slot under DEVIT_WGRADFR=0 (not taken)
    tail_one_token    2 x 197, 1, 256 / 4 / 512: D != 384, never a job even when a slot is offered
    tail_compacted    3 x 51, 2, 384 / 4 (attn_width 256) / 640: every Da-versus-D offset and leading dimension differs
    tail_short        4 x 6, 2, 384 / 6 / 768: fewer keys than one attention tile
    tail_two_tiles    130 x 6, 2, 384 / 6 / 768: T = 260 crosses a row tile, Tp = 512
    tail_wide_tokens  2 x 198, 40, 384 / 6 / 1536: several query rows per image in the rows-form backward"""
import ctypes as C
import math

import torch

import _attn_model as A
import _drop_model as DM
import _gemm_model as G
import _tail_model as T
from _tail_model import BF16, F16, F32, F64, U, gen, ratio, stored16   # noqa: F401

EPS = 1e-6
SAVE, QKV_PAD, ATT = 1, 2, 4
ACT_NAMES = ("ln1", "mean1", "rstd1", "qkv", "attn_o", "lse", "x1", "att", "ln2", "mean2", "rstd2", "h", "h_pre", "x2")
BWD_NAMES = ("dh_pre", "dln2", "dx1", "g1", "dattn", "dqkv", "dln1", "lnws")
ACC_NAMES = ("n1w", "n1b", "qkv_w", "qkv_b", "proj_w", "proj_b", "n2w", "n2b", "fc1_w", "fc1_b", "fc2_w", "fc2_b")
ENV_SWITCHES = ("DEVIT_GEMMFR", "DEVIT_WGRADFR", "DEVIT_WGRAD_STREAM", "DEVIT_LNFUSE", "DEVIT_GEMM4", "DEVIT_WGRAD_GROUP")
ERR_SHAPE, ERR_ARG = -1, -2

MUTATIONS = {  # planted wiring bug -> the stage (or untouched-bytes check) that must see it
    "ln2_reads_x": "ln2", "x2_residual_from_x": "x2", "dp2_for_dp1": "x1", "h_pre_after_gate": "h_pre", "proj_bias_twice": "x1",
    "pad_rows_left": "pad_rows", "fc2_bias_twice": "fc2_b", "proj_b_from_dx1": "proj_b", "g_prev_unscaled": "g_prev",
    "dqkv_add_dropped": "dqkv", "lse_not_saved_per_head": "lse", "dx_pingpong_stale": "inputs"}
# the dropped sequence's planted wiring bugs -> (stage, what the rates must be for the bug to change anything: 'p', 'p_attn' or 'p != p_attn')
DROP_MUTATIONS = {
    "site2_mask_at_site4": ("x2", "p"), "bwd_site3_left_out": ("dh_pre", "p"), "attn_scale_at_site2": ("x1", "p != p_attn"),
    "attn_pitch_N": ("attn_o", "p_attn"), "bwd_mask_of_next_block": ("g1", "p"), "fc2_b_from_unmasked_g2": ("fc2_b", "p"),
    "proj_b_by_layernorm_too": ("proj_b", "p"), "x2_from_proj_tmp": ("x2", "p"), "h_pre_masked_too": ("h_pre", "p"),
    "g2_masked_out_of_place": ("inputs/g2", "p"), "fc2_w_reads_unmasked_h": ("fc2_w", "p")}
MUTATIONS.update({k: v[0] for k, v in DROP_MUTATIONS.items()})


def _case(name, B, N, D, heads, hidden, flags, dtype16=0, fc2t=False, envs=(("", {}),)):
    return dict(name=name, B=B, N=N, D=D, heads=heads, hidden=hidden, flags=flags, dtype16=dtype16, fc2t=fc2t, envs=envs)


CASES = [
    _case("student", 2, 198, 384, 6, 1536, SAVE | QKV_PAD | ATT),
    _case("student_fr", 2, 198, 384, 6, 1536, SAVE | QKV_PAD | ATT, fc2t=True, envs=(("", {"DEVIT_GEMMFR": "1"}),)),
    _case("compacted", 3, 51, 384, 4, 640, SAVE | QKV_PAD,
          envs=(("", {}), ("gemmfr", {"DEVIT_GEMMFR": "1"}), ("wgradfr0", {"DEVIT_WGRADFR": "0"}))),
    _case("wide", 2, 197, 256, 4, 512, SAVE | ATT, envs=(("", {}), ("wgrad_stream0", {"DEVIT_WGRAD_STREAM": "0"}))),
    _case("short", 4, 17, 384, 6, 768, SAVE | QKV_PAD),
    _case("f16_fwd", 1, 208, 256, 4, 512, QKV_PAD | ATT, dtype16=1),
]


# ---- the dropped sequence (devit_encoder_fwd_drop / devit_block_bwd_drop: block_fwd / block_bwd with d != NULL).  A case names the block index its
# masks are generated for; a run is (tag, environment, (p, p_attn)).  DEVIT_BLK_ATT is refused under p > 0, so no case carries it.
DROP_SEED = (0x9E3779B9 << 32) | 20240807


def drop_of(block, p, p_attn, seed=DROP_SEED):
    """the per-block dropout description of the audit and of emulate(): what devit_block_dropout carries, as rates"""
    return dict(seed=seed, block=block, p=p, p_attn=p_attn)


DROP_CASES = [
    dict(_case("student_drop", 2, 198, 384, 6, 1536, SAVE | QKV_PAD), block=5, runs=(("", {}, (0.1, 0.1)),)),
    dict(_case("student_fr_drop", 2, 198, 384, 6, 1536, SAVE | QKV_PAD, fc2t=True), block=0, runs=(("", {"DEVIT_GEMMFR": "1"}, (0.5, 0.0)),)),
    dict(_case("compacted_drop", 3, 51, 384, 4, 640, SAVE | QKV_PAD), block=11,
         runs=(("attn", {}, (0.0, 0.25)), ("attn/wgradfr0", {"DEVIT_WGRADFR": "0"}, (0.0, 0.25)), ("both", {}, (0.1, 0.1)),
               ("both/wgradfr0", {"DEVIT_WGRADFR": "0"}, (0.1, 0.1)))),
    dict(_case("wide_drop", 2, 197, 256, 4, 512, SAVE), block=5,
         runs=(("", {}, (0.1, 0.1)), ("wgrad_stream0", {"DEVIT_WGRAD_STREAM": "0"}, (0.1, 0.1)))),
]


def drop_variants():
    """(id, case, environment, dropout description) of every run of the dropped table"""
    return [(c["name"] + ("/" + tag if tag else ""), c, env, drop_of(c["block"], *rates)) for c in DROP_CASES for tag, env, rates in c["runs"]]


def case_named(name):
    return next(c for c in CASES + DROP_CASES if c["name"] == name)


def variants(backward_only=False):
    """(id, case, environment) of every run of the table"""
    out = []
    for c in CASES:
        if backward_only and not c["flags"] & SAVE:
            continue
        for tag, env in c["envs"]:
            out.append((c["name"] + ("/" + tag if tag else ""), c, env))
    return out


def set_env(monkeypatch, env):
    """every per-call switch of the sequence cleared, then the variant's own set"""
    for k in ENV_SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def pad_rows(m):
    return (m + 255) // 256 * 256


def qkv_extra(c):
    return (128 if c["N"] >= 128 else 256 - c["N"]) if c["flags"] & QKV_PAD else 0


def dims(c):
    M = c["B"] * c["N"]
    return dict(B=c["B"], N=c["N"], D=c["D"], H=c["heads"], Da=64 * c["heads"], Hd=c["hidden"], M=M, Mp=pad_rows(M))


# ============================================================================================ buffer extents as include/devit_hip.h words them
def act_extents(c):
    """bytes per DEVIT_ACT_* buffer: "bf16 row buffers have pad_rows(M) rows (qkv: + the overhang when flagged)"; mean / rstd [M], lse [B][H][N] and
    the fc1 pre-activation only with DEVIT_BLK_SAVE; x1 / x2 fp32 [M][D]; att bf16 [M][D] only with DEVIT_BLK_ATT"""
    d = dims(c)
    M, Mp, D, Da, Hd = d["M"], d["Mp"], d["D"], d["Da"], d["Hd"]
    save, att = bool(c["flags"] & SAVE), bool(c["flags"] & ATT)
    stat = M * 4 if save else 0
    return dict(ln1=Mp * D * 2, mean1=stat, rstd1=stat, qkv=(Mp + qkv_extra(c)) * 3 * Da * 2, attn_o=Mp * Da * 2,
                lse=d["B"] * d["H"] * d["N"] * 4 if save else 0, x1=M * D * 4, att=M * D * 2 if att else 0, ln2=Mp * D * 2, mean2=stat, rstd2=stat,
                h=Mp * Hd * 2, h_pre=Mp * Hd * 2 if save else 0, x2=M * D * 4)


def bwd_extents(c):
    """bytes per DEVIT_BWD_* buffer; the LayerNorm workspace is devit_layernorm_bwd_workspace(M, D) = grid x 3 x D floats (layernorm.hip:208)"""
    d = dims(c)
    M, Mp, D, Da, Hd = d["M"], d["Mp"], d["D"], d["Da"], d["Hd"]
    return dict(dh_pre=Mp * Hd * 2, dln2=Mp * D * 2, dx1=M * D * 4, g1=Mp * D * 2, dattn=Mp * Da * 2, dqkv=Mp * 3 * Da * 2, dln1=Mp * D * 2,
                lnws=T.ln_bwd_grid(M) * 3 * D * 4)


def buffer_shapes(c):
    """name -> (rows, cols, 16-bit?) of every buffer a block forward / backward writes, as the sequence addresses them"""
    d = dims(c)
    M, Mp, D, Da, Hd = d["M"], d["Mp"], d["D"], d["Da"], d["Hd"]
    return dict(ln1=(Mp, D, 1), mean1=(1, M, 0), rstd1=(1, M, 0), qkv=(Mp + qkv_extra(c), 3 * Da, 1), attn_o=(Mp, Da, 1),
                lse=(d["B"] * d["H"], d["N"], 0), x1=(M, D, 0), att=(M, D, 1), ln2=(Mp, D, 1), mean2=(1, M, 0), rstd2=(1, M, 0), h=(Mp, Hd, 1),
                h_pre=(Mp, Hd, 1), x2=(M, D, 0), dh_pre=(Mp, Hd, 1), dln2=(Mp, D, 1), dx1=(M, D, 0), g1=(Mp, D, 1), dattn=(Mp, Da, 1),
                dqkv=(Mp, 3 * Da, 1), dln1=(Mp, D, 1))


PADDED = ("ln1", "qkv", "attn_o", "ln2", "h", "h_pre", "dh_pre", "dln2", "g1", "dattn", "dqkv", "dln1", "g_prev")     # 16-bit, rows >= M zeroed


# ============================================================================================ inputs
def _mix(vals, n, shift):
    return torch.tensor([vals[(i + shift) % len(vals)] for i in range(n)], dtype=F32)


def dp_scales(B, shift=0):
    """(dp1, dp2) [B]: different per-image vectors from the existing mixes, each with a 0 and a value above 1 where B >= 2"""
    if B == 1:
        return torch.tensor([1.25]), torch.tensor([0.5])
    return _mix((1.25, 0.0, 1.0 / 0.9, 1.0), B, shift), _mix((0.0, 2.0, 0.5, 1.0), B, shift)


def block_weights(c, key=0):
    """seeded parameters of one block: 16-bit GEMM weights (bf16 / f16 values), nonzero fp32 biases, gammas off 1, betas off 0, gates from the
    existing mixes (head: 0.5, 2, 0, 1; neuron: 0, 1, 0.5, -1.5, 3)"""
    d = dims(c)
    D, Da, Hd, H = d["D"], d["Da"], d["Hd"], d["H"]
    g = gen("block", c["name"], "w", key)
    dt = F16 if c["dtype16"] else BF16
    rn = lambda *s: T.randn(g, *s)                                                              # noqa: E731
    w = dict(n1w=1 + 0.1 * rn(D), n1b=0.1 * rn(D), n2w=1 + 0.1 * rn(D), n2b=0.1 * rn(D),
             qkv_w16=(rn(3 * Da, D) / math.sqrt(D) * 2).to(dt), qkv_b=0.2 * rn(3 * Da), proj_w16=(rn(D, Da) / math.sqrt(Da)).to(dt), proj_b=0.2 * rn(D),
             fc1_w16=(rn(Hd, D) / math.sqrt(D) * 2).to(dt), fc1_b=0.3 * rn(Hd), fc2_w16=(rn(D, Hd) / math.sqrt(Hd)).to(dt), fc2_b=0.2 * rn(D))
    w["head_gate"] = _mix(A.GATE_MIX, H, key)
    w["neuron_gate"] = torch.tensor(G.COLSCALES)[torch.randint(0, 5, (Hd,), generator=g)]
    w["dp1"], w["dp2"] = dp_scales(d["B"], key)
    if c["fc2t"]:
        w["fc2_w16t"] = w["fc2_w16"].t().contiguous()
    return w


def inputs(c, key=0, dqkv_add=True):
    """seeded CPU tensors of one block forward + backward: w (block_weights), x with a per-row offset, dx, g2 = bf16(dp2 dx), dqkv_add (or None),
    prev_dp2, and acc0: what every gradient accumulator (prev_fc2_b included) holds before the call -- the sequence accumulates"""
    d = dims(c)
    M, D, Da, Hd, B = d["M"], d["D"], d["Da"], d["Hd"], d["B"]
    g = gen("block", c["name"], "x", key)
    w = block_weights(c, key)
    x = T.randn(g, M, D) + 2 * T.randn(g, M, 1)
    dx = T.randn(g, M, D)
    inp = dict(w=w, x=x, dx=dx, g2=(dx * w["dp2"].repeat_interleave(d["N"])[:, None]).to(BF16),
               dqkv_add=(0.5 * T.randn(g, M, 3 * Da)).to(BF16) if dqkv_add else None, prev_dp2=_mix(T.ROWSCALE_MIX, B, key + 1))
    shapes = dict(n1w=(D,), n1b=(D,), qkv_w=(3 * Da, D), qkv_b=(3 * Da,), proj_w=(D, Da), proj_b=(D,), n2w=(D,), n2b=(D,), fc1_w=(Hd, D),
                  fc1_b=(Hd,), fc2_w=(D, Hd), fc2_b=(D,), prev_fc2_b=(D,))
    inp["acc0"] = {k: 3 * T.randn(g, *s) for k, s in shapes.items()}
    return inp


def to_device(inp, dev):
    mv = lambda v: v.to(dev) if isinstance(v, torch.Tensor) else ({k: mv(x) for k, x in v.items()} if isinstance(v, dict) else v)   # noqa: E731
    return mv(inp)


# ============================================================================================ which launch produced what
def colsum_pass_roundings(rows):
    """devit_colsum_bf16 on `rows` rows (elementwise.hip): 64 chunks from 512 rows on, else 1 (:462); a thread adds every 8th row of its chunk in
    sequence (:220-233), 8 partials of the workgroup (:242); sum_partials_kernel: every 8th chunk in sequence (:254), 8 groups (:260), the
    accumulate (:261)"""
    nchunk = 64 if rows >= 512 else 1
    per = -(-rows // nchunk)
    return -(-per // 8) + 8 + -(-nchunk // 8) + 8 + 1


def colsum_pass_bounds(y16, rows, out0):
    """column sums of the live rows of a bf16 matrix as the column-sum pass over `rows` (padded) rows adds them -> (float64 sums + out0, bound)"""
    v = y16.to(F64)
    ref = T.colsum_ref(v, v.shape[0], v.shape[1], 0, 0).to(v.device) + out0.to(F64)
    return ref, U * colsum_pass_roundings(rows) * (v.abs().sum(0) + out0.to(F64).abs())


def routes(c, env, lnws_bytes, colsum_ws, fused=(False, False), g2_bias_done=False, prev=True, drop=None):
    """The decisions of block_bwd (csrc/encoder.hip) that change WHICH kernel an output comes from, hence how many roundings its bound counts:
    wmode (the grouped launch: D == 384, three K-steps, DEVIT_WGRADFR != 0) and who owns fc2's bias gradient: 'handed' (g2_bias_done: not this
    call's), 'colsum' (the pass over g2, when the LayerNorm workspace is large enough for it) or 'launch' (the row sums of fc2's own split-K
    launch).  fused: devit_dgrad_layernorm_bwd_fused at the LN2 and LN1 sites, asked of the library by the caller.  prev: g_prev / prev_fc2_b given.
    drop with p > 0: 'masked' -- the column sums of the site-4 pass over g2, whatever the other rules would say (block_bwd: fc2_bias_here = false)."""
    d = dims(c)
    wmode = d["D"] == 384 and d["Mp"] // 64 >= 3 and env.get("DEVIT_WGRADFR", "1") != "0"
    fb = "handed" if g2_bias_done else "colsum" if (wmode and d["Hd"] % 128 == 0 and lnws_bytes >= colsum_ws) else "launch"
    if drop is not None and drop["p"] > 0:
        assert not g2_bias_done, "devit_block_bwd_drop refuses g2_bias_done with p > 0"
        fb = "masked"
    return dict(wmode=wmode, fc2_bias=fb, fused=tuple(fused), prev=prev)


def default_routes(c, env=None, **kw):
    """routes() from the restated extents (no library needed: the CPU tests)"""
    return routes(c, env or {}, bwd_extents(c)["lnws"], 64 * c["D"] * 4, **kw)


def fused_chain(tiles):
    """longest chain of additions of the fused launch's column sums (tests/test_gpu_lnfuse.py, chain_length)"""
    return 32 + 1 + 3 + -(-tiles // 32) + 32 + 1


# ============================================================================================ the stages
def _rs(v, N):
    return v.to(F64).repeat_interleave(N)[:, None]


def _d(t):
    return t.to(F64)


def _ln_fwd_stage(tag, x, gamma, beta, y16, mean, rstd, f16, save):
    r, b = T.ln_fwd_bounds(x, gamma, beta, EPS)
    yield "ln" + tag, y16, r["y"], stored16(b["y"], r["y"], f16)
    if save:
        yield "mean" + tag, mean, r["mean"], b["mean"]
        yield "rstd" + tag, rstd, r["rstd"], b["rstd"]


# ---- the dropout passes.  Masks come from the numpy mirror alone (tests/_philox.py through _drop_model._keep and _attn_model.attn_keep), thr / s
# from _drop_model.thr_s; every bound is one the sibling models already state, composed where a pass rewrites a stage's buffer in place.
SITE_ATTN, SITE_PROJ, SITE_HIDDEN, SITE_FC2 = 1, 2, 3, 4
_ATTN_KEEP = {}


def is_dropped(drop):
    """(drop, drop_attn) of block_fwd / block_bwd: thr > 0, thr_attn > 0"""
    return (False, False) if drop is None else (DM.thr_s(drop["p"])[0] > 0, DM.thr_s(drop["p_attn"])[0] > 0)


def site_keep(c, drop, site, cols, dev="cpu", block=None):
    """bool [M][cols], pitch cols: the keep mask of sites 2, 3, 4 of the block (another block's with `block`)"""
    blk = drop["block"] if block is None else block
    return DM._keep(drop["seed"], site, blk, DM.thr_s(drop["p"])[0], dims(c)["M"], cols, cols).to(dev)


def attn_site_keep(c, drop, dev="cpu", pitch=None):
    """bool [B][H][N][N] at pitch ceil4(N) (or the pitch a wrong kernel would take), and scale_keep_attn"""
    d = dims(c)
    key = (drop["seed"], drop["block"], drop["p_attn"], d["B"], d["H"], d["N"], pitch)
    if key not in _ATTN_KEEP:
        _ATTN_KEEP[key] = A.attn_keep(drop["seed"], drop["block"], DM.thr_s(drop["p_attn"])[0], d["B"], d["H"], d["N"], pitch=pitch)
    return _ATTN_KEEP[key].to(dev), DM.thr_s(drop["p_attn"])[1]


def _apply_case(drop, site, rows, cols, p=None, colsum=False):
    return dict(kernel="apply", dtype=BF16, rows=rows, cols=cols, ld=cols, pitch=cols, colsum=colsum, site=site, block=drop["block"],
                p=drop["p"] if p is None else p, seed=drop["seed"])


def masked16(drop, site, pre16, keep):
    """_drop_model.apply_statement of a bf16 buffer's live rows: what devit_dropout_apply must leave of them, to the bit"""
    z = torch.zeros(pre16.shape[1], dtype=F32, device=pre16.device)
    return DM.apply_statement(_apply_case(drop, site, *pre16.shape), dict(x=pre16, colsum0=z), keep)[0]


def masked_colsum_bounds(drop, site, stored16_, out0):
    """the column sums devit_dropout_apply adds to its `colsum` while it masks, stated on the buffer AS STORED (apply_statement at p = 0 keeps every
    element's bits, so its sums and its bound -- strip + 3 + gy additions, _drop_model's docstring -- are those of the stored values) + the preload"""
    keep = torch.ones(stored16_.shape, dtype=torch.bool, device=stored16_.device)
    _, colsum, bound = DM.apply_statement(_apply_case(drop, site, *stored16_.shape, p=0.0, colsum=True), dict(x=stored16_, colsum0=out0), keep)
    return colsum, bound


def masked_in_place(drop, ref, e, keep):
    """A 16-bit buffer a launch wrote and devit_dropout_apply then rewrote in place: the launch's statement gives (ref, e), its 16-bit store included.
    A dropped element is the zero apply_statement states (bound 0).  A kept one is bf16(fp32(v) * s) of the stored v, |v - ref| <= e
    (dropout_apply_kernel.inc:32: one fp32 product, one rounding to bf16; :21 is the fp32 buffers' line): around s ref it lies within
        s e  +  stored16(U s (|ref| + e), s (|ref| + e))
    -- the producer's error scaled, plus apply's own two roundings on an input of magnitude |ref| + e."""
    s = DM.thr_s(drop["p"])[1]
    mag = s * (ref.abs() + e)
    zero = torch.zeros((), dtype=F64, device=ref.device)
    return torch.where(keep, s * ref, zero), torch.where(keep, s * e + stored16(U * mag, mag), zero)


def residual_stage(c, drop, site, x, y, rowscale, keep, got, e_y=None):
    """devit_dropout_residual (x_out = x + rowscale y s where kept) -> (float64 reference, bound): _drop_model.residual_statement and judge_residual's
    bound 2^-24 (|rs y s| + |out|); bound 0 (x's value exactly) where the element is dropped or its row scale is 0.  e_y: y is itself a float64
    statement with this bound, of a temporary that is gone -- its error reaches the output times |rs| s"""
    d = dims(c)
    rc = dict(kernel="residual", rows=d["M"], cols=x.shape[1], rps=d["N"], p=drop["p"], site=site)
    want, branch, exact = DM.residual_statement(rc, dict(x=x, y=y, rowscale=rowscale), keep)
    bound = DM.U24 * (branch.abs() + got.to(F64).abs())
    if e_y is not None:
        bound = bound + _rs(rowscale, d["N"]).abs() * DM.thr_s(drop["p"])[1] * e_y
    return want, torch.where(exact, torch.zeros((), dtype=F64, device=bound.device), bound)


def _attn_drop_kw(c, drop, dev, pitch=None):
    if not is_dropped(drop)[1]:
        return {}
    keep, s = attn_site_keep(c, drop, dev, pitch)
    return dict(keep=keep, s=s)


def forward_stages(c, inp, bufs, drop=None):
    """yields (stage, got, float64 reference, bound) for what devit_encoder_fwd (with `drop`: devit_encoder_fwd_drop) left of one block, read off
    block_fwd"""
    d, w = dims(c), inp["w"]
    B, N, H, M = d["B"], d["N"], d["H"], d["M"]
    f16, save = bool(c["dtype16"]), bool(c["flags"] & SAVE)
    x = bufs["x"]
    dev = x.device
    yield from _ln_fwd_stage("1", x, w["n1w"], w["n1b"], bufs["ln1"][:M], bufs.get("mean1"), bufs.get("rstd1"), f16, save)
    ref, bnd = G.statement(G.STORE_BF16, _d(bufs["ln1"][:M]), _d(w["qkv_w16"]), bias=_d(w["qkv_b"]), f16=f16)
    yield "qkv", bufs["qkv"][:M], ref["out"], bnd["out"]
    q, k, v, _, _ = A.split_packed(bufs["qkv"], B, N, H)
    r, b = A.bounds(q, k, v, w["head_gate"], 0.125, u=A.U_F16 if f16 else A.U_BF16, f16=f16, **_attn_drop_kw(c, drop, dev))
    yield "attn_o", A.heads(bufs["attn_o"], B, N, H), r["O"], b["O"]
    if save:
        yield "lse", bufs["lse"].view(B, H, N), r["lse"], b["lse"]
    yield from branch_forward_stages(c, inp, bufs, x, (M, d["Mp"], N), drop)


def branch_forward_stages(c, inp, bufs, x, geo, drop=None):
    """the branch half of the forward (branch_fwd in csrc/encoder.hip), from the proj GEMM on, on geo = (rows, padded rows, rows per DropPath scale) of
    `x` and of the buffers: the block's own (dims(c)["M"], ["Mp"], ["N"]) with x = bufs["x"], the lean last block's (B ntok, pad_rows(B ntok), ntok)
    with x = the gathered token rows.  The dropout passes are the block's alone."""
    d, w = dims(c), inp["w"]
    M, _, N = geo
    D, Hd = d["D"], d["Hd"]
    f16, save, att = bool(c["dtype16"]), bool(c["flags"] & SAVE), bool(c["flags"] & ATT)
    dropped, _ = is_dropped(drop)
    assert not dropped or (M, N) == (d["M"], d["N"])
    dev = x.device
    if dropped:      # proj stores fp32 into the temporary fc2 then overwrites: its statement and the residual pass's (site 2) compose
        ref, bnd = G.statement(G.STORE_F32, _d(bufs["attn_o"][:M]), _d(w["proj_w16"]), bias=_d(w["proj_b"]))
        yield ("x1", bufs["x1"]) + residual_stage(c, drop, SITE_PROJ, bufs["x"], ref["out"], w["dp1"], site_keep(c, drop, SITE_PROJ, D, dev), bufs["x1"],
                                                  bnd["out"])
    else:
        ref, bnd = G.statement(G.RESIDUAL, _d(bufs["attn_o"][:M]), _d(w["proj_w16"]), bias=_d(w["proj_b"]), res=_d(x), rowscale=_rs(w["dp1"], N), aux=att,
                               f16=f16)
        yield "x1", bufs["x1"], ref["out"], bnd["out"]
        if att:
            yield "att", bufs["att"], ref["aux"], bnd["aux"]
    yield from _ln_fwd_stage("2", bufs["x1"], w["n2w"], w["n2b"], bufs["ln2"][:M], bufs.get("mean2"), bufs.get("rstd2"), f16, save)
    ref, bnd = G.statement(G.GELU, _d(bufs["ln2"][:M]), _d(w["fc1_w16"]), bias=_d(w["fc1_b"]), colscale=_d(w["neuron_gate"]), aux=save, f16=f16)
    if dropped:      # masked in place after the GELU launch (site 3); the saved pre-activation stays as the launch left it
        yield ("h", bufs["h"][:M]) + masked_in_place(drop, ref["out"], bnd["out"], site_keep(c, drop, SITE_HIDDEN, Hd, dev))
    else:
        yield "h", bufs["h"][:M], ref["out"], bnd["out"]
    if save:
        yield "h_pre", bufs["h_pre"][:M], ref["aux"], bnd["aux"]
    if dropped:      # fc2 stores fp32 into the temporary (as the call leaves it), the residual pass forms x2 from the stored x1 and tmp (site 4)
        ref, bnd = G.statement(G.STORE_F32, _d(bufs["h"][:M]), _d(w["fc2_w16"]), bias=_d(w["fc2_b"]))
        keep4 = site_keep(c, drop, SITE_FC2, D, dev)
        if bufs.get("tmp") is not None:
            yield "tmp", bufs["tmp"][:M], ref["out"], bnd["out"]
            yield ("x2", bufs["x2"]) + residual_stage(c, drop, SITE_FC2, bufs["x1"], bufs["tmp"][:M], w["dp2"], keep4, bufs["x2"])
        else:        # a block of a chain whose successor has written the shared temporary since: composed as x1 is
            yield ("x2", bufs["x2"]) + residual_stage(c, drop, SITE_FC2, bufs["x1"], ref["out"], w["dp2"], keep4, bufs["x2"], bnd["out"])
        return
    ref, bnd = G.statement(G.RESIDUAL, _d(bufs["h"][:M]), _d(w["fc2_w16"]), bias=_d(w["fc2_b"]), res=_d(bufs["x1"]), rowscale=_rs(w["dp2"], N), f16=f16)
    yield "x2", bufs["x2"], ref["out"], bnd["out"]


def _live(buf, M, Mp):
    """the [Mp][cols] operand a weight-gradient reduction is STATED on: the live rows, zero below -- junk the sequence left in a pad row is then in
    what the launch summed and not in the reference"""
    out = torch.zeros((Mp, buf.shape[1]), dtype=F64, device=buf.device)
    out[:M] = buf[:M].to(F64)
    return out


def _wgrad_stage(name, bname, dy, x, w0, b0, M, Mp, route):
    """w_grad [Nw][Kf] += dy^T x (+ b_grad += column sums of dy from the same launch when b0 is given), by the launch wgrad_job / linear_wgrad
    (csrc/encoder.hip) send it to: a job of the grouped launch (the most slices split_k == 0 can choose), else the split-K launch"""
    from devit_amd import ops
    Nw, Kf = w0.shape
    dyl, xl = _live(dy, M, Mp), _live(x, M, Mp)
    job = None
    if route["wmode"] and Kf == 384 and Nw % 128 == 0:
        job = dict(a=dyl, b=xl, a_cols=Nw, transposed=0)
    elif route["wmode"] and Nw == 384 and Kf % 128 == 0 and b0 is None:
        job = dict(a=xl, b=dyl, a_cols=Kf, transposed=1)
    if job is not None:
        dd = dict(job=dict(a_cols=job["a_cols"], transposed=job["transposed"]), a=job["a"], b=job["b"], out0=w0.reshape(-1), ldc=Kf, orows=Nw, ocols=Kf)
        if b0 is not None:
            dd["colsum0"] = b0
        ref, bnd = G.wgrad_reference(dd, Mp, G.wgrad_max_split(Mp))
        return [(name, ref["out"], bnd["out"])] + ([(bname, ref["colsum"], bnd["colsum"])] if b0 is not None else [])
    ref, bnd = G.statement(G.ATOMIC, dyl.t(), xl.t(), out0=_d(w0), aux0=None if b0 is None else _d(b0), aux=b0 is not None,
                           split_k=ops.split_k_for(Nw, Kf, Mp // 64), tiles_n=Kf // 128)
    return [(name, ref["out"], bnd["out"])] + ([(bname, ref["aux"], bnd["aux"])] if b0 is not None else [])


def _ln_bwd_stage(tag, x, mean, rstd, gamma, dln, dres, g0, b0, M, fused, tiles):
    r, b = T.ln_bwd_bounds(x, mean, rstd, gamma, dln, dres, g0, b0)
    if fused:        # the same terms in the fused launch's order: the longer chain of the two (tests/test_gpu_lnfuse.py)
        nc, nf = T.ln_col_roundings(M), max(T.ln_col_roundings(M), fused_chain(tiles))
        b = dict(b, dgamma=b["dgamma"] * (nf + 3) / (nc + 3), dbeta=b["dbeta"] * nf / nc)
    return r, b


def backward_stages(c, inp, bufs, route, dln=None, drop=None):
    """yields (stage, got, float64 reference, bound) for what devit_block_bwd (with `drop`: devit_block_bwd_drop) left, read off block_bwd.  route:
    routes().  dln: {'dln2': .., 'dln1': ..} the LayerNorm backward's input where the fused launch kept it on chip (from a run of the two launches on
    bit-identical dh_pre / dqkv).  Under p > 0 bufs['g2'] is the caller's buffer as the call left it: masked (audit() holds it to the pre-mask value)."""
    d, w, a0 = dims(c), inp["w"], inp["acc0"]
    B, N, H, M, Mp, Da = d["B"], d["N"], d["H"], d["M"], d["Mp"], d["Da"]
    tiles = Mp // 256
    acc = bufs["acc"]
    dev = bufs["dx"].device
    yield from branch_backward_stages(c, inp, bufs, route, (M, Mp, N), dln, drop)
    # 9
    add = bufs.get("dqkv_add")
    q, k, v, do, ad = A.split_packed(bufs["qkv"], B, N, H, bufs["dattn"], add)
    r, b = A.bounds(q, k, v, w["head_gate"], 0.125, do, ad, **_attn_drop_kw(c, drop, dev))
    got = torch.stack([A.heads(bufs["dqkv"], B, N, H, j * Da) for j in range(3)])
    yield "dqkv", got, torch.stack([r["dQ"], r["dK"], r["dV"]]), torch.stack([b["dQ"], b["dK"], b["dV"]])
    # 10
    if not route["fused"][1]:
        ref, bnd = G.statement(G.STORE_BF16, _d(bufs["dqkv"][:M]), _d(w["qkv_w16"]).t())
        yield "dln1", bufs["dln1"][:M], ref["out"], bnd["out"]
    # 11
    for name, ref, bnd in _wgrad_stage("qkv_w", "qkv_b", bufs["dqkv"], bufs["ln1"], a0["qkv_w"], a0["qkv_b"], M, Mp, route):
        yield name, acc[name], ref, bnd
    # 12
    dln1 = (dln or bufs)["dln1"] if route["fused"][1] else bufs["dln1"]
    r, b = _ln_bwd_stage("1", bufs["x"], bufs["mean1"], bufs["rstd1"], w["n1w"], dln1[:M], bufs["dx1"], a0["n1w"], a0["n1b"], M, route["fused"][1], tiles)
    yield "dx_in", bufs["dx_in"], r["dx"], b["dx"]
    yield "n1w", acc["n1w"], r["dgamma"], b["dgamma"]
    yield "n1b", acc["n1b"], r["dbeta"], b["dbeta"]
    if route["prev"]:
        ref = _rs(inp["prev_dp2"], N) * _d(bufs["dx_in"])
        yield "g_prev", bufs["g_prev"][:M], ref, stored16(U * ref.abs(), ref)
        if "prev_fc2_b" in acc:
            ref, bnd = T.ln_colsum_bounds(bufs["g_prev"][:M], a0["prev_fc2_b"])
            if route["fused"][1]:
                bnd = bnd * max(T.ln_col_roundings(M), fused_chain(tiles)) / T.ln_col_roundings(M)
            yield "prev_fc2_b", acc["prev_fc2_b"], ref, bnd


def branch_backward_stages(c, inp, bufs, route, geo, dln=None, drop=None):
    """the branch half of the backward (branch_bwd in csrc/encoder.hip: stages 1 to 8, up to proj's dgrad and weight gradient) on geo = (rows, padded
    rows, rows per DropPath scale), as branch_forward_stages.  route: wmode / fc2_bias / fused[0] of the Ctx the half ran on."""
    d, w, a0 = dims(c), inp["w"], inp["acc0"]
    M, Mp, N = geo
    D, Hd = d["D"], d["Hd"]
    tiles = Mp // 256
    acc = bufs["acc"]
    g2, dx = bufs["g2"], bufs["dx"]
    dropped, _ = is_dropped(drop)
    assert not dropped or (M, N) == (d["M"], d["N"])
    dev = dx.device
    assert dropped == (route["fc2_bias"] == "masked")
    # 1, 2: fc2's weight gradient and who owns its bias gradient
    own = route["fc2_bias"] == "launch"
    st = _wgrad_stage("fc2_w", "fc2_b", g2, bufs["h"], a0["fc2_w"], a0["fc2_b"] if own else None, M, Mp, route)
    if route["fc2_bias"] == "colsum":
        ref, bnd = colsum_pass_bounds(g2[:M], Mp, a0["fc2_b"])
        yield "fc2_b", acc["fc2_b"], ref, bnd
    elif route["fc2_bias"] == "handed":
        yield "fc2_b", acc["fc2_b"], _d(a0["fc2_b"]), torch.zeros_like(_d(a0["fc2_b"]))
    elif route["fc2_bias"] == "masked":      # the site-4 pass's own column sums of what it stored, and nothing else
        yield ("fc2_b", acc["fc2_b"]) + masked_colsum_bounds(drop, SITE_FC2, g2[:M], a0["fc2_b"])
    for name, ref, bnd in st[::-1]:
        yield name, acc[name], ref, bnd
    # 3
    ref, bnd = G.statement(G.DGELU, _d(g2[:M]), _d(w["fc2_w16"]).t(), colscale=_d(w["neuron_gate"]), aux_in=_d(bufs["h_pre"][:M]))
    if dropped:      # masked in place after the dGELU launch (site 3)
        yield ("dh_pre", bufs["dh_pre"][:M]) + masked_in_place(drop, ref["out"], bnd["out"], site_keep(c, drop, SITE_HIDDEN, Hd, dev))
    else:
        yield "dh_pre", bufs["dh_pre"][:M], ref["out"], bnd["out"]
    # 4
    if not route["fused"][0]:
        ref, bnd = G.statement(G.STORE_BF16, _d(bufs["dh_pre"][:M]), _d(w["fc1_w16"]).t())
        yield "dln2", bufs["dln2"][:M], ref["out"], bnd["out"]
    # 5
    for name, ref, bnd in _wgrad_stage("fc1_w", "fc1_b", bufs["dh_pre"], bufs["ln2"], a0["fc1_w"], a0["fc1_b"], M, Mp, route):
        yield name, acc[name], ref, bnd
    # 6
    dln2 = (dln or bufs)["dln2"] if route["fused"][0] else bufs["dln2"]
    r, b = _ln_bwd_stage("2", bufs["x1"], bufs["mean2"], bufs["rstd2"], w["n2w"], dln2[:M], dx, a0["n2w"], a0["n2b"], M, route["fused"][0], tiles)
    yield "dx1", bufs["dx1"], r["dx"], b["dx"]
    if dropped:
        # The pre-mask value is bf16(dp1 * dx1) of the STORED dx1: one fp32 product, one rounding -- torch's product, to which tests/test_gpu_tail.py
        # (the LayerNorm backward) and tests/test_gpu_lnfuse.py (the fused launch) hold this output bit for bit.  The equality carries over on both
        # routes, so the masked g1 is held to apply_statement of it (site 2) bit for bit: the bound is 0.
        pre = (w["dp1"].to(F32).repeat_interleave(N)[:, None] * bufs["dx1"]).to(BF16)
        want = masked16(drop, SITE_PROJ, pre, site_keep(c, drop, SITE_PROJ, D, dev)).to(F64)
        yield "g1", bufs["g1"][:M], want, torch.zeros_like(want)
    else:
        ref = _rs(w["dp1"], N) * _d(bufs["dx1"])
        yield "g1", bufs["g1"][:M], ref, stored16(U * ref.abs(), ref)
    yield "n2w", acc["n2w"], r["dgamma"], b["dgamma"]
    yield "n2b", acc["n2b"], r["dbeta"], b["dbeta"]
    if dropped:      # the LayerNorm backward ran with a NULL column-sum pointer: the site-2 pass's sums of the masked g1, and nothing else
        ref, bnd = masked_colsum_bounds(drop, SITE_PROJ, bufs["g1"][:M], a0["proj_b"])
    else:
        ref, bnd = T.ln_colsum_bounds(bufs["g1"][:M], a0["proj_b"])
        if route["fused"][0]:
            bnd = bnd * max(T.ln_col_roundings(M), fused_chain(tiles)) / T.ln_col_roundings(M)
    yield "proj_b", acc["proj_b"], ref, bnd
    # 7
    ref, bnd = G.statement(G.STORE_BF16, _d(bufs["g1"][:M]), _d(w["proj_w16"]).t())
    yield "dattn", bufs["dattn"][:M], ref["out"], bnd["out"]
    # 8
    for name, ref, bnd in _wgrad_stage("proj_w", None, bufs["g1"], bufs["attn_o"], a0["proj_w"], None, M, Mp, route):
        yield name, acc[name], ref, bnd


def audit(c, inp, bufs, route=None, dln=None, drop=None):
    """-> ({stage: worst |err| / bound over every live element}, problems): problems names every untouched-bytes statement that does not hold --
    'pad_rows/<buffer>' (a 16-bit buffer whose rows >= M are not zero, the qkv overhang included), 'inputs/<name>' (an input of the call that
    did not come back bit for bit).  route None: the forward alone.  drop (drop_of()): the dropped sequence; with p > 0 the caller's g2 is the one
    input that must NOT come back as it was: it must be torch.equal to apply_statement of the value the test handed in (site 4)."""
    M, D = dims(c)["M"], dims(c)["D"]
    rt = {}
    for name, got, ref, bnd in forward_stages(c, inp, bufs, drop):
        rt[name] = ratio(got, ref, bnd)
    if route is not None:
        for name, got, ref, bnd in backward_stages(c, inp, bufs, route, dln, drop):
            rt[name] = ratio(got, ref, bnd)
    problems = []
    for name in PADDED:
        t = bufs.get(name)
        if t is not None and t.shape[0] > M and bool((t[M:].view(torch.int16) != 0).any()):
            problems.append("pad_rows/" + name)
    for name in ("x", "dx", "g2", "dqkv_add"):
        if bufs.get(name) is None or inp.get(name) is None:
            continue
        want = inp[name]
        if name == "g2" and route is not None and is_dropped(drop)[0]:
            want = masked16(drop, SITE_FC2, want, site_keep(c, drop, SITE_FC2, D, want.device))
        if not torch.equal(bufs[name][:want.shape[0]].cpu(), want.cpu()):
            problems.append("inputs/" + name)
    return rt, problems


# ============================================================================================ emulation
def _emu_apply(t16, keep, s):
    """devit_dropout_apply on a bf16 buffer's live rows: bf16(fp32(x) * s) where kept, +0 where dropped"""
    return torch.where(keep, (t16.to(F32) * torch.tensor(s, dtype=F32)).to(BF16), torch.zeros((), dtype=BF16))


def _emu_residual(x, y, rs, keep, s):
    """devit_dropout_residual as _drop_model.emulate_residual words it: t = y * s rounded, out = fmaf(rs, t, x) where kept, x's bits where dropped"""
    t = y * torch.tensor(s, dtype=F32)
    return torch.where(keep, (rs.to(F64) * t.to(F64) + x.to(F64)).to(F32), x)


def _f32(t):
    return t.to(F32)


def _padded(v, M, Mp, t, extra=0):
    """a buffer of Mp (+ extra) rows as the sequence leaves it: the live rows stored in `t`, zeros below"""
    out = torch.zeros((Mp + extra, v.shape[1]), dtype=t)
    out[:M] = v.to(t)
    return out


def _emu_drop_state(c, drop):
    """what the emulated branch halves share of the dropped sequence: the masks of sites 2, 3, 4 and scale_keep (the forward half adds what the
    mutations of the backward half read: proj's temporary, the unmasked h)"""
    st = dict(dropped=is_dropped(drop)[0])
    if st["dropped"]:
        st["s_keep"] = DM.thr_s(drop["p"])[1]
        st["keep2"], st["keep3"], st["keep4"] = (site_keep(c, drop, site, cols)
                                                 for site, cols in ((SITE_PROJ, c["D"]), (SITE_HIDDEN, c["hidden"]), (SITE_FC2, c["D"])))
    return st


def _emu_branch_fwd(c, inp, bufs, x, geo, dp1, dp2, mutate, drop, st):
    """branch_fwd emulated on geo = (rows, padded rows, rows per DropPath scale): from bufs['attn_o'] and the fp32 rows `x` to x1, ln2, mean2, rstd2,
    h, h_pre, x2 (att, tmp).  dp1 / dp2: the scale of every row, [rows][1]."""
    w = inp["w"]
    M, Mp, _ = geo
    f16, att = bool(c["dtype16"]), bool(c["flags"] & ATT)
    dt = F16 if f16 else BF16
    dropped = st["dropped"]
    f = _f32
    padded = lambda v: _padded(v, M, Mp, dt)                                                    # noqa: E731
    pre = f(bufs["attn_o"][:M]) @ f(w["proj_w16"]).t() + w["proj_b"]
    if mutate == "proj_bias_twice":
        pre = pre + w["proj_b"]
    if dropped:
        s_keep, keep2, keep3, keep4 = st["s_keep"], st["keep2"], st["keep3"], st["keep4"]
        st["tmp_proj"] = tmp_proj = pre
        bufs["x1"] = _emu_residual(x, pre, dp1, keep2, DM.thr_s(drop["p_attn"])[1] if mutate == "attn_scale_at_site2" else s_keep)
    else:
        bufs["x1"] = x + dp1 * pre
    if att:
        bufs["att"] = pre.to(dt)
    e = T.ln_fwd_emulate(x if mutate == "ln2_reads_x" else bufs["x1"], w["n2w"], w["n2b"], EPS)
    bufs.update(ln2=padded(e["y"]), mean2=e["mean"], rstd2=e["rstd"])
    pre = f(bufs["ln2"][:M]) @ f(w["fc1_w16"]).t() + w["fc1_b"]
    bufs["h"] = padded(G.gelu_fit32(pre) * w["neuron_gate"])
    bufs["h_pre"] = padded(pre * w["neuron_gate"] if mutate == "h_pre_after_gate" else pre)
    if dropped:
        st["h_unmasked"] = bufs["h"].clone()
        bufs["h"][:M] = _emu_apply(bufs["h"][:M], keep3, s_keep)
        if mutate == "h_pre_masked_too":
            bufs["h_pre"][:M] = _emu_apply(bufs["h_pre"][:M], keep3, s_keep)
        bufs["tmp"] = torch.full((Mp, c["D"]), math.nan, dtype=F32)      # (rows >= M are never written: whatever the arena held)
        bufs["tmp"][:M] = f(bufs["h"][:M]) @ f(w["fc2_w16"]).t() + w["fc2_b"]
        bufs["x2"] = _emu_residual(x if mutate == "x2_residual_from_x" else bufs["x1"], tmp_proj if mutate == "x2_from_proj_tmp" else bufs["tmp"][:M],
                                   dp2, keep2 if mutate == "site2_mask_at_site4" else keep4, s_keep)
    else:
        bufs["x2"] = (x if mutate == "x2_residual_from_x" else bufs["x1"]) + dp2 * (f(bufs["h"][:M]) @ f(w["fc2_w16"]).t() + w["fc2_b"])


def _emu_branch_bwd(c, inp, bufs, acc, geo, dp1, mutate, drop, st, route):
    """branch_bwd emulated on geo, as _emu_branch_fwd: from dx and the caller's g2 (inp['dx'], inp['g2']: the live rows) to fc2 / fc1 / proj's
    gradients, n2w / n2b, dh_pre, dln2, dx1, g1, dattn; bufs['dx'] and bufs['g2'] as the call leaves the caller's buffers' live rows"""
    w, a0 = inp["w"], inp["acc0"]
    M, Mp, _ = geo
    D_ = c["D"]
    dropped = st["dropped"]
    f = _f32
    padded = lambda v: _padded(v, M, Mp, BF16)                                                  # noqa: E731
    dx, g2 = inp["dx"], padded(inp["g2"])
    if dropped:      # site 4: the caller's g2 masked in place, its column sums are fc2's bias gradient
        assert route["fc2_bias"] == "masked", "routes(..., drop=...)"
        s_keep, keep2, keep3, keep4 = st["s_keep"], st["keep2"], st["keep3"], st["keep4"]
        g2_unmasked = g2
        g2 = padded(_emu_apply(inp["g2"], keep4, s_keep))
    bufs.update(dx=dx.clone(), g2=inp["g2"].clone() if (not dropped or mutate == "g2_masked_out_of_place") else g2[:M].clone())
    if mutate == "pad_rows_left":
        bufs["h"][Mp - 2] = 0.375
    if route["fc2_bias"] == "handed":
        acc["fc2_b"] = a0["fc2_b"].clone()
    elif mutate == "fc2_b_from_unmasked_g2":
        acc["fc2_b"] = a0["fc2_b"] + f(g2_unmasked).sum(0)
    else:
        acc["fc2_b"] = a0["fc2_b"] + f(g2).sum(0) * (2 if mutate == "fc2_bias_twice" else 1)
    acc["fc2_w"] = a0["fc2_w"] + f(g2).t() @ f(st["h_unmasked"] if mutate == "fc2_w_reads_unmasked_h" else bufs["h"])
    dh = (f(g2[:M]) @ f(w["fc2_w16"])) * w["neuron_gate"] * G.dgelu_fit32(f(bufs["h_pre"][:M]))
    bufs["dh_pre"] = padded(dh)
    if dropped and mutate != "bwd_site3_left_out":
        bufs["dh_pre"][:M] = _emu_apply(bufs["dh_pre"][:M], keep3, s_keep)
    bufs["dln2"] = padded(f(bufs["dh_pre"][:M]) @ f(w["fc1_w16"]))
    acc["fc1_w"] = a0["fc1_w"] + f(bufs["dh_pre"]).t() @ f(bufs["ln2"])
    acc["fc1_b"] = a0["fc1_b"] + f(bufs["dh_pre"]).sum(0)
    e = T.ln_bwd_emulate(bufs["x1"], bufs["mean2"], bufs["rstd2"], w["n2w"], bufs["dln2"][:M], dx, a0["n2w"], a0["n2b"])
    bufs["dx1"], acc["n2w"], acc["n2b"] = e["dx"], e["dgamma"], e["dbeta"]
    bufs["g1"] = padded(dp1 * bufs["dx1"])
    ln_sums = f(bufs["g1"][:M]).sum(0)       # what the LayerNorm backward would add, given a column-sum pointer
    if dropped:      # site 2
        kb = site_keep(c, drop, SITE_PROJ, D_, block=drop["block"] + 1) if mutate == "bwd_mask_of_next_block" else keep2
        bufs["g1"][:M] = _emu_apply(bufs["g1"][:M], kb, s_keep)
    acc["proj_b"] = a0["proj_b"] + (bufs["dx1"] if mutate == "proj_b_from_dx1" else f(bufs["g1"][:M])).sum(0)
    if mutate == "proj_b_by_layernorm_too":
        acc["proj_b"] = acc["proj_b"] + ln_sums
    if mutate == "pad_rows_left":
        bufs["g1"][M] = -0.75
    bufs["dattn"] = padded(f(bufs["g1"][:M]) @ f(w["proj_w16"]))
    acc["proj_w"] = a0["proj_w"] + f(bufs["g1"]).t() @ f(bufs["attn_o"])


def emulate(c, inp, mutate=None, route=None, drop=None):
    """One block forward (and, with DEVIT_BLK_SAVE, backward) in fp32 torch, every buffer of the sequence as it would be left -> bufs as audit()
    takes them.  The GEMMs are plain fp32 products (another order than the kernels'), LayerNorm and attention are the sibling models' emulations,
    16-bit stores one rounding.  `mutate`: one of MUTATIONS, a planted WIRING bug -- every kernel stays correct.  drop (drop_of()): the dropped
    sequence, with bufs['tmp'] as fc2 leaves it and bufs['g2'] masked in place."""
    assert mutate is None or mutate in MUTATIONS
    assert mutate not in DROP_MUTATIONS or drop is not None
    st = _emu_drop_state(c, drop)
    akw = _attn_drop_kw(c, drop, "cpu", pitch=c["N"] if mutate == "attn_pitch_N" else None)
    d, w, a0 = dims(c), inp["w"], inp["acc0"]
    B, N, H, M, Mp, Da = d["B"], d["N"], d["H"], d["M"], d["Mp"], d["Da"]
    f16, save = bool(c["dtype16"]), bool(c["flags"] & SAVE)
    dt = F16 if f16 else BF16
    route = route or default_routes(c)
    f = lambda t: t.to(F32)                                                                     # noqa: E731

    def padded(v, extra=0, t=dt):
        out = torch.zeros((Mp + extra, v.shape[1]), dtype=t)
        out[:M] = v.to(t)
        return out

    x = inp["x"]
    dp1 = (w["dp2"] if mutate == "dp2_for_dp1" else w["dp1"]).repeat_interleave(N)[:, None]
    dp2 = w["dp2"].repeat_interleave(N)[:, None]
    bufs = dict(x=x.clone())
    e = T.ln_fwd_emulate(x, w["n1w"], w["n1b"], EPS)
    bufs.update(ln1=padded(e["y"]), mean1=e["mean"], rstd1=e["rstd"])
    bufs["qkv"] = padded(f(bufs["ln1"][:M]) @ f(w["qkv_w16"]).t() + w["qkv_b"], qkv_extra(c))
    q, k, v, _, _ = A.split_packed(bufs["qkv"], B, N, H)
    ae = A.emulate(q, k, v, w["head_gate"], 0.125, f16=f16, **akw)
    bufs["attn_o"] = padded(A.rows(ae["O"]))
    lse = ae["lse"].to(F32)
    if mutate == "lse_not_saved_per_head":
        lse = lse[:, :1].expand(B, H, N).contiguous()
    bufs["lse"] = lse
    _emu_branch_fwd(c, inp, bufs, x, (M, Mp, N), dp1, dp2, mutate, drop, st)
    if not save:
        for k_ in ("mean1", "rstd1", "lse", "mean2", "rstd2", "h_pre"):
            del bufs[k_]
        return bufs
    # ---- backward
    acc = {}
    _emu_branch_bwd(c, inp, bufs, acc, (M, Mp, N), dp1, mutate, drop, st, route)
    bufs["dqkv_add"] = inp["dqkv_add"]
    add = None if (inp["dqkv_add"] is None or mutate == "dqkv_add_dropped") else inp["dqkv_add"]
    q, k, v, do, ad = A.split_packed(bufs["qkv"], B, N, H, bufs["dattn"], add)
    ae = A.emulate(q, k, v, w["head_gate"], 0.125, do, ad, **akw)
    bufs["dqkv"] = padded(torch.cat([A.rows(ae[n]) for n in ("dQ", "dK", "dV")], 1), t=BF16)
    bufs["dln1"] = padded(f(bufs["dqkv"][:M]) @ f(w["qkv_w16"]), t=BF16)
    acc["qkv_w"] = a0["qkv_w"] + f(bufs["dqkv"]).t() @ f(bufs["ln1"])
    acc["qkv_b"] = a0["qkv_b"] + f(bufs["dqkv"]).sum(0)
    e = T.ln_bwd_emulate(x, bufs["mean1"], bufs["rstd1"], w["n1w"], bufs["dln1"][:M], bufs["dx1"], a0["n1w"], a0["n1b"])
    bufs["dx_in"], acc["n1w"], acc["n1b"] = e["dx"], e["dgamma"], e["dbeta"]
    if route["prev"]:
        pdp = 1.0 if mutate == "g_prev_unscaled" else inp["prev_dp2"].repeat_interleave(N)[:, None]
        bufs["g_prev"] = padded(pdp * bufs["dx_in"], t=BF16)
        acc["prev_fc2_b"] = a0["prev_fc2_b"] + f(bufs["g_prev"][:M]).sum(0)
    if mutate == "dx_pingpong_stale":       # dx_in written over the dx the block was given: every output is right, the caller's buffer is not
        bufs["dx"] = bufs["dx_in"].clone()
    bufs["acc"] = acc
    return bufs


# ============================================================================================ the C structs of a call
def structs(c, adr, flags=None):
    """(devit_block_weights, devit_block_acts, devit_block_wgrads, devit_block_bwd_io) of a case.  adr(name) -> the address that stands for the named
    buffer or None: weights by their field name, 'x', 'dp1', 'dp2', the DEVIT_ACT_* / DEVIT_BWD_* buffers by ACT_NAMES / BWD_NAMES,
    'g_<accumulator>', 'dx', 'g2', 'dx_in', 'g_prev', 'prev_dp2', 'g_prev_fc2_b', 'dqkv_add' (and 'tmp', the dropped sequence's fp32 temporary: refused())"""
    from devit_amd import _lib as L
    d = dims(c)
    w = L.BlockWeights()
    for n in ("n1w", "n1b", "qkv_b", "proj_b", "n2w", "n2b", "fc1_b", "fc2_b", "qkv_w16", "proj_w16", "fc1_w16", "fc2_w16", "head_gate", "neuron_gate"):
        setattr(w, n, adr(n))
    w.num_heads, w.attn_width, w.hidden, w.dtype16 = d["H"], d["Da"], d["Hd"], c["dtype16"]
    w.fc2_w16t = adr("fc2_w16t") if c["fc2t"] else None
    a = L.BlockActs()
    a.x, a.dp1, a.dp2, a.flags = adr("x"), adr("dp1"), adr("dp2"), c["flags"] if flags is None else flags
    for i, n in enumerate(ACT_NAMES):
        a.buf[i] = adr(n)
    g = L.BlockWgrads()
    for n in ACC_NAMES:
        setattr(g, n, adr("g_" + n))
    io = L.BlockBwdIO()
    io.dx, io.g2, io.dx_in, io.g_prev = adr("dx"), adr("g2"), adr("dx_in"), adr("g_prev")
    io.prev_dp2, io.prev_fc2_b_grad, io.g2_bias_done, io.dqkv_add = adr("prev_dp2"), adr("g_prev_fc2_b"), 0, adr("dqkv_add")
    for i, n in enumerate(BWD_NAMES):
        io.ws[i] = adr(n)
    io.lnws_bytes = 0
    io.defer_jobs = io.defer_count = None
    return w, a, g, io


def call_fwd(nblocks, w, a, c, stream=None):
    """devit_encoder_fwd itself (no raise) -> (return code, message)"""
    from devit_amd import _lib as L
    lib = L.load()
    rc = lib.devit_encoder_fwd(nblocks, w, a, c["B"], c["N"], c["D"], EPS, stream)
    return rc, lib.devit_last_error().decode() if rc else ""


def call_bwd(w, a, g, io, c, stream=None):
    from devit_amd import _lib as L
    lib = L.load()
    ref = lambda s: None if s is None else C.byref(s)                                           # noqa: E731
    rc = lib.devit_block_bwd(ref(w), ref(a), ref(g), ref(io), c["B"], c["N"], c["D"], EPS, stream)
    return rc, lib.devit_last_error().decode() if rc else ""


def drop_struct(drop, tmp):
    """devit_block_dropout of a description: thr / s of both rates from _drop_model.thr_s, `tmp` the address of the shared fp32 temporary or None"""
    from devit_amd import _lib as L
    s = L.BlockDropout()
    (thr, sk), (thr_a, sk_a) = DM.thr_s(drop["p"]), DM.thr_s(drop["p_attn"])
    s.seed, s.block, s.thr, s.thr_attn, s.scale_keep, s.scale_keep_attn, s.tmp = drop["seed"], drop["block"], thr, thr_a, sk, sk_a, tmp
    return s


def call_fwd_drop(nblocks, w, a, dr, c, stream=None):
    """devit_encoder_fwd_drop itself (no raise) -> (return code, message); dr: the devit_block_dropout array (or one struct by reference) or None"""
    from devit_amd import _lib as L
    lib = L.load()
    rc = lib.devit_encoder_fwd_drop(nblocks, w, a, dr, c["B"], c["N"], c["D"], EPS, stream)
    return rc, lib.devit_last_error().decode() if rc else ""


def call_bwd_drop(w, a, g, io, dr, c, stream=None):
    from devit_amd import _lib as L
    lib = L.load()
    ref = lambda s: None if s is None else C.byref(s)                                           # noqa: E731
    rc = lib.devit_block_bwd_drop(ref(w), ref(a), ref(g), ref(io), ref(dr), c["B"], c["N"], c["D"], EPS, stream)
    return rc, lib.devit_last_error().decode() if rc else ""


def _set(obj, **kw):
    for k, v in kw.items():
        setattr(obj, k, v)


def _null_buf(arr, i):
    arr[i] = None


# (name, case, what to change in (case copy, w, a, g, io) before the call, which entry point, DEVIT_ERR_*, words the message must hold).  'fwd2': two
# blocks, `change` sees the second block's acts.  Every one is an argument check in front of the first launch (csrc/encoder.hip).
REFUSALS = [
    ("N_209", "student", lambda c, w, a, g, io: c.update(N=209), "fwd", ERR_SHAPE, "N=209"),
    ("D_320", "student", lambda c, w, a, g, io: c.update(D=320), "fwd", ERR_SHAPE, "D=320"),
    ("N_209_bwd", "student", lambda c, w, a, g, io: c.update(N=209), "bwd", ERR_SHAPE, "N=209"),
    ("attn_width_not_64_heads", "student", lambda c, w, a, g, io: _set(w, num_heads=5), "fwd", ERR_SHAPE, "heads 5 * 64"),
    ("attn_width_not_64_heads_bwd", "student", lambda c, w, a, g, io: _set(w, num_heads=5), "bwd", ERR_SHAPE, "heads 5 * 64"),
    ("f16_with_save", "f16_fwd", lambda c, w, a, g, io: _set(a, flags=a.flags | SAVE), "fwd", ERR_ARG, "f16 is the frozen-teacher forward"),
    ("null_activation_buffer", "student", lambda c, w, a, g, io: _null_buf(a.buf, ACT_NAMES.index("ln2")), "fwd", ERR_ARG, "null activation buffer"),
    ("null_saved_buffer", "student", lambda c, w, a, g, io: _null_buf(a.buf, ACT_NAMES.index("lse")), "fwd", ERR_ARG, "DEVIT_BLK_SAVE needs"),
    ("att_flag_without_att", "student", lambda c, w, a, g, io: _null_buf(a.buf, ACT_NAMES.index("att")), "fwd", ERR_ARG, "DEVIT_BLK_ATT needs att"),
    ("second_block_reads_another_x", "student", lambda c, w, a, g, io: None, "fwd2", ERR_ARG, "block 1 does not read block 0's output"),
    ("backward_without_save", "student", lambda c, w, a, g, io: _set(a, flags=a.flags & ~SAVE), "bwd", ERR_ARG, "without DEVIT_BLK_SAVE"),
    ("f16_backward", "f16_fwd", lambda c, w, a, g, io: _set(a, flags=a.flags | SAVE), "bwd", ERR_ARG, "f16 blocks have no backward"),
    ("null_workspace_entry", "student", lambda c, w, a, g, io: _null_buf(io.ws, BWD_NAMES.index("dattn")), "bwd", ERR_ARG, "workspace 4 is null"),
    ("null_accumulator", "student", lambda c, w, a, g, io: _set(g, proj_b=None), "bwd", ERR_ARG, "null gradient accumulator"),
    ("null_g2", "student", lambda c, w, a, g, io: _set(io, g2=None), "bwd", ERR_ARG, "dx / g2 / dx_in"),
    ("null_io", "student", lambda c, w, a, g, io: None, "bwd_null_io", ERR_ARG, "null argument"),
    # the _drop entry points ('fwd_drop' / 'bwd_drop'): c["dr"] is the call's devit_block_dropout, (0.1, 0.1) at the case's block, tmp given
    ("null_dropout_array", "student_drop", lambda c, w, a, g, io: c.update(dr=None), "fwd_drop", ERR_ARG, "null dropout array"),
    ("null_dropout_bwd", "student_drop", lambda c, w, a, g, io: c.update(dr=None), "bwd_drop", ERR_ARG, "null dropout"),
    ("drop_without_tmp", "student_drop", lambda c, w, a, g, io: _set(c["dr"], tmp=None), "fwd_drop", ERR_ARG, "p > 0 needs the fp32 temporary"),
    ("drop_with_att", "student", lambda c, w, a, g, io: None, "fwd_drop", ERR_ARG, "cannot also store the attention-branch output (DEVIT_BLK_ATT)"),
    ("drop_on_f16", "f16_fwd", lambda c, w, a, g, io: None, "fwd_drop", ERR_ARG, "dropout runs on bf16 blocks"),
    ("attn_drop_on_f16", "f16_fwd", lambda c, w, a, g, io: _set(c["dr"], thr=0), "fwd_drop", ERR_ARG, "dropout runs on bf16 blocks"),
    ("drop_block_negative", "student_drop", lambda c, w, a, g, io: _set(c["dr"], block=-1), "fwd_drop", ERR_ARG, "dropout runs on bf16 blocks"),
    ("drop_block_negative_bwd", "student_drop", lambda c, w, a, g, io: _set(c["dr"], block=-1), "bwd_drop", ERR_ARG, "block -1"),
    ("attn_drop_block_negative_bwd", "student_drop", lambda c, w, a, g, io: _set(c["dr"], block=-1, thr=0), "bwd_drop", ERR_ARG, "block -1"),
    ("g2_bias_done_with_drop", "student_drop", lambda c, w, a, g, io: _set(io, g2_bias_done=1), "bwd_drop", ERR_ARG, "g2_bias_done must be 0"),
    ("drop_on_f16_bwd", "f16_fwd", lambda c, w, a, g, io: _set(a, flags=a.flags | SAVE), "bwd_drop", ERR_ARG, "f16 blocks have no backward"),
]


# ---- the lean last block (devit_tail_fwd / devit_tail_bwd, include/devit_hip.h): the block's buffers on T = B ntok rows from the attention output
# on, (K | V) in the qkv slot, and three buffers of its own; the backward's transients likewise, with two of its own
TAIL_ACT_NAMES = ACT_NAMES + ("ln1_tok", "q", "x_tok")
TAIL_BWD_NAMES = BWD_NAMES + ("dkv", "dln1_tok")
# (B, N, ntok, D, attn_width, hidden): one row tile, the student's last block, a compacted one
TAIL_SIZE_CASES = ((3, 5, 1, 128, 128, 128), (2, 198, 2, 384, 384, 1536), (2, 198, 2, 384, 256, 1024))


def tail_extents(B, N, ntok, D, Da, Hd, save):
    """(bytes per devit_tail_acts buffer, bytes per devit_tail_bwd transient) as the header words them"""
    M, Tr = B * N, B * ntok
    Mp, Tp = pad_rows(M), pad_rows(Tr)
    acts = dict(ln1=Mp * D * 2, mean1=M * 4 * save, rstd1=M * 4 * save, qkv=Mp * 2 * Da * 2, attn_o=Tp * Da * 2, lse=B * (Da // 64) * ntok * 4 * save,
                x1=Tr * D * 4, att=0, ln2=Tp * D * 2, mean2=Tr * 4 * save, rstd2=Tr * 4 * save, h=Tp * Hd * 2, h_pre=Tp * Hd * 2 * save, x2=Tr * D * 4,
                ln1_tok=Tp * D * 2, q=Tp * Da * 2, x_tok=Tr * D * 4)
    bwd = dict(dh_pre=Tp * Hd * 2, dln2=Tp * D * 2, dx1=Tr * D * 4, g1=Tp * D * 2, dattn=Tp * Da * 2, dqkv=Tp * 3 * Da * 2, dln1=Mp * D * 2,
               lnws=T.ln_bwd_grid(M) * 3 * D * 4, dkv=Mp * 2 * Da * 2, dln1_tok=Tp * D * 2)
    return acts, bwd


def tail_library_sizes(B, N, ntok, D, Da, Hd, flags):
    from devit_amd import _lib as L
    sa, sb = (C.c_size_t * len(TAIL_ACT_NAMES))(), (C.c_size_t * len(TAIL_BWD_NAMES))()
    L.call("devit_tail_acts_sizes", B, N, ntok, D, Da, Hd, flags, sa)
    L.call("devit_tail_bwd_sizes", B, N, ntok, D, Da, Hd, sb)
    return dict(zip(TAIL_ACT_NAMES, sa)), dict(zip(TAIL_BWD_NAMES, sb))


def tail_structs(c, adr, ntok=2):
    """(devit_block_weights, devit_tail_acts, devit_block_wgrads, devit_tail_bwd_io) of a case, addresses as for structs()"""
    from devit_amd import _lib as L
    w, a, g, _ = structs(c, adr, flags=c["flags"] & SAVE)
    t = L.TailActs()
    t.acts = a
    t.acts.buf[ACT_NAMES.index("att")] = None
    t.ln1_tok, t.q, t.x_tok, t.ntok = adr("ln1_tok"), adr("q"), adr("x_tok"), ntok
    io = L.TailBwdIO()
    io.dx, io.g2, io.dx_in, io.lnws_bytes = adr("dx"), adr("g2"), adr("dx_in"), 0
    for i, n in enumerate(TAIL_BWD_NAMES):
        io.ws[i] = adr(n)
    io.defer_jobs = io.defer_count = None
    return w, t, g, io


# as REFUSALS, for 'tail_fwd' / 'tail_bwd' (`a` is the devit_tail_acts, `io` the devit_tail_bwd_io) and 'copy' (c["copy"]: the arguments of
# devit_token_rows_copy behind the two pointers, by name).  Every one in front of the first launch, the memsets included.
TAIL_REFUSALS = [
    ("tail_null_acts", "student", lambda c, w, a, g, io: c.update(null="a"), "tail_fwd", ERR_ARG, "null argument"),
    ("tail_N_209", "student", lambda c, w, a, g, io: c.update(N=209), "tail_fwd", ERR_SHAPE, "N=209"),
    ("tail_D_320", "student", lambda c, w, a, g, io: c.update(D=320), "tail_fwd", ERR_SHAPE, "D=320"),
    ("tail_heads", "student", lambda c, w, a, g, io: _set(w, num_heads=5), "tail_fwd", ERR_SHAPE, "heads 5 * 64"),
    ("tail_ntok_0", "student", lambda c, w, a, g, io: _set(a, ntok=0), "tail_fwd", ERR_SHAPE, "ntok=0"),
    ("tail_ntok_above_N", "student", lambda c, w, a, g, io: _set(a, ntok=199), "tail_fwd", ERR_SHAPE, "ntok=199 of N=198"),
    ("tail_flag_att", "student", lambda c, w, a, g, io: _set(a.acts, flags=SAVE | ATT), "tail_fwd", ERR_ARG, "DEVIT_BLK_SAVE is the only one"),
    ("tail_f16_with_save", "f16_fwd", lambda c, w, a, g, io: _set(a.acts, flags=SAVE), "tail_fwd", ERR_ARG, "f16 is the frozen-teacher forward"),
    ("tail_null_block_buffer", "student", lambda c, w, a, g, io: _null_buf(a.acts.buf, ACT_NAMES.index("ln2")), "tail_fwd", ERR_ARG, "null activation buffer"),
    ("tail_null_q", "student", lambda c, w, a, g, io: _set(a, q=None), "tail_fwd", ERR_ARG, "null activation buffer"),
    ("tail_null_x_tok", "student", lambda c, w, a, g, io: _set(a, x_tok=None), "tail_fwd", ERR_ARG, "null activation buffer"),
    ("tail_null_saved_buffer", "student", lambda c, w, a, g, io: _null_buf(a.acts.buf, ACT_NAMES.index("rstd2")), "tail_fwd", ERR_ARG, "DEVIT_BLK_SAVE needs"),
    ("tail_bwd_null_io", "student", lambda c, w, a, g, io: c.update(null="io"), "tail_bwd", ERR_ARG, "null argument"),
    ("tail_bwd_N_209", "student", lambda c, w, a, g, io: c.update(N=209), "tail_bwd", ERR_SHAPE, "N=209"),
    ("tail_bwd_heads", "student", lambda c, w, a, g, io: _set(w, num_heads=5), "tail_bwd", ERR_SHAPE, "heads 5 * 64"),
    ("tail_bwd_ntok_above_N", "student", lambda c, w, a, g, io: _set(a, ntok=199), "tail_bwd", ERR_SHAPE, "ntok=199 of N=198"),
    ("tail_bwd_without_save", "student", lambda c, w, a, g, io: _set(a.acts, flags=0), "tail_bwd", ERR_ARG, "without DEVIT_BLK_SAVE"),
    ("tail_bwd_f16", "f16_fwd", lambda c, w, a, g, io: _set(a.acts, flags=SAVE), "tail_bwd", ERR_ARG, "f16 blocks have no backward"),
    ("tail_bwd_null_accumulator", "student", lambda c, w, a, g, io: _set(g, qkv_b=None), "tail_bwd", ERR_ARG, "null gradient accumulator"),
    ("tail_bwd_null_dx_in", "student", lambda c, w, a, g, io: _set(io, dx_in=None), "tail_bwd", ERR_ARG, "dx / g2 / dx_in"),
    ("tail_bwd_null_dkv", "student", lambda c, w, a, g, io: _null_buf(io.ws, TAIL_BWD_NAMES.index("dkv")), "tail_bwd", ERR_ARG, "workspace 8 is null"),
    ("tail_bwd_null_dattn", "student", lambda c, w, a, g, io: _null_buf(io.ws, TAIL_BWD_NAMES.index("dattn")), "tail_bwd", ERR_ARG, "workspace 4 is null"),
    ("copy_null_src", "student", lambda c, w, a, g, io: c["copy"].update(src=None), "copy", ERR_ARG, "null pointer"),
    ("copy_elem_3", "student", lambda c, w, a, g, io: c["copy"].update(elem=3), "copy", ERR_ARG, "elem=3"),
    ("copy_add_16_bit", "student", lambda c, w, a, g, io: c["copy"].update(add=1), "copy", ERR_ARG, "add=1 on 16-bit"),
    ("copy_unaligned_src", "student", lambda c, w, a, g, io: c["copy"].update(src=c["copy"]["src"] + 8), "copy", ERR_ARG, "whole 16-byte vectors"),
    ("copy_unaligned_dst", "student", lambda c, w, a, g, io: c["copy"].update(dst=c["copy"]["dst"] + 2), "copy", ERR_ARG, "whole 16-byte vectors"),
    ("copy_unaligned_src_ld", "student", lambda c, w, a, g, io: c["copy"].update(src_ld=388), "copy", ERR_ARG, "whole 16-byte vectors"),
    ("copy_unaligned_dst_ld", "student", lambda c, w, a, g, io: c["copy"].update(dst_ld=1156), "copy", ERR_ARG, "whole 16-byte vectors"),
    ("copy_cols_not_whole_vectors", "student", lambda c, w, a, g, io: c["copy"].update(cols=380), "copy", ERR_ARG, "whole 16-byte vectors"),
    ("copy_ntok_above_rows", "student", lambda c, w, a, g, io: c["copy"].update(ntok=3), "copy", ERR_SHAPE, "ntok=3"),
    ("copy_cols_above_ld", "student", lambda c, w, a, g, io: c["copy"].update(cols=392), "copy", ERR_SHAPE, "cols=392"),
]
REFUSALS += TAIL_REFUSALS


def _refused_tail(c, change, entry, adr0):
    from devit_amd import _lib as L
    lib = L.load()
    # (the lean block's own buffers stand at block buffers of the same kind: a refused call touches none of them)
    stand_in = dict(ln1_tok="ln2", q="attn_o", x_tok="x1", dkv="dqkv", dln1_tok="dln2")
    adr = lambda n: adr0(stand_in.get(n, n))                                                    # noqa: E731
    w, t, g, io = tail_structs(c, adr)
    c["copy"] = dict(src=adr("x"), src_rows_per_image=198, src_ld=384, dst=adr("x_tok"), dst_rows_per_image=2, dst_ld=1152, B=2, ntok=2, cols=384,
                     elem=2, add=0)
    change(c, w, t, g, io)
    ref = lambda s, n: None if c.get("null") == n else C.byref(s)                               # noqa: E731
    if entry == "tail_fwd":
        rc = lib.devit_tail_fwd(ref(w, "w"), ref(t, "a"), c["B"], c["N"], c["D"], EPS, None)
    elif entry == "tail_bwd":
        rc = lib.devit_tail_bwd(ref(w, "w"), ref(t, "a"), ref(g, "g"), ref(io, "io"), c["B"], c["N"], c["D"], EPS, None)
    else:
        k = c["copy"]
        rc = lib.devit_token_rows_copy(k["src"], k["src_rows_per_image"], k["src_ld"], k["dst"], k["dst_rows_per_image"], k["dst_ld"], k["B"],
                                       k["ntok"], k["cols"], k["elem"], k["add"], None)
    return rc, lib.devit_last_error().decode() if rc else ""


def refused(case_name, change, entry, adr):
    """run one REFUSALS row with the addresses adr() gives -> (return code, message)"""
    from devit_amd import _lib as L
    c = dict(case_named(case_name))
    if entry in ("tail_fwd", "tail_bwd", "copy"):
        return _refused_tail(c, change, entry, adr)
    w, a, g, io = structs(c, adr)
    c["dr"] = drop_struct(drop_of(c.get("block", 0), 0.1, 0.1), adr("tmp"))
    change(c, w, a, g, io)
    if entry == "fwd_drop":
        return call_fwd_drop(1, C.byref(w), C.byref(a), None if c["dr"] is None else C.byref(c["dr"]), c)
    if entry == "bwd_drop":
        return call_bwd_drop(w, a, g, io, c["dr"], c)
    if entry == "fwd":
        return call_fwd(1, C.byref(w), C.byref(a), c)
    if entry == "fwd2":
        ws, as_ = (L.BlockWeights * 2)(w, w), (L.BlockActs * 2)(a, a)        # the second block reads the first's x, not its x2
        return call_fwd(2, ws, as_, c)
    if entry == "bwd_null_io":
        return call_bwd(w, a, g, None, c)
    return call_bwd(w, a, g, io, c)


def sizes_refusals():
    """the two sizes functions: a null `sizes` pointer, N = 209, D = 320 -> [(name, return code, message, expected code, words)]"""
    from devit_amd import _lib as L
    lib = L.load()
    out = []
    sa, sb = (C.c_size_t * len(ACT_NAMES))(), (C.c_size_t * len(BWD_NAMES))()
    for name, args, sz_a, sz_b, code, words in (("null_sizes", (2, 198, 384, 384, 1536), None, None, ERR_ARG, "null"),
                                               ("N_209", (2, 209, 384, 384, 1536), sa, sb, ERR_SHAPE, "N=209"),
                                               ("D_320", (2, 198, 320, 384, 1536), sa, sb, ERR_SHAPE, "D=320")):
        rc = lib.devit_block_acts_sizes(*args, SAVE, sz_a)
        out.append(("acts_sizes/" + name, rc, lib.devit_last_error().decode(), code, words))
        rc = lib.devit_block_bwd_sizes(*args, sz_b)
        out.append(("bwd_sizes/" + name, rc, lib.devit_last_error().decode(), code, words))
    ta, tb = (C.c_size_t * len(TAIL_ACT_NAMES))(), (C.c_size_t * len(TAIL_BWD_NAMES))()
    for name, args, sz_a, sz_b, code, words in (("null_sizes", (2, 198, 2, 384, 384, 1536), None, None, ERR_ARG, "null"),
                                               ("N_209", (2, 209, 2, 384, 384, 1536), ta, tb, ERR_SHAPE, "N=209"),
                                               ("ntok_0", (2, 198, 0, 384, 384, 1536), ta, tb, ERR_SHAPE, "ntok=0"),
                                               ("ntok_above_N", (2, 5, 6, 384, 384, 1536), ta, tb, ERR_SHAPE, "ntok=6 of N=5")):
        rc = lib.devit_tail_acts_sizes(*args, SAVE, sz_a)
        out.append(("tail_acts_sizes/" + name, rc, lib.devit_last_error().decode(), code, words))
        rc = lib.devit_tail_bwd_sizes(*args, sz_b)
        out.append(("tail_bwd_sizes/" + name, rc, lib.devit_last_error().decode(), code, words))
    return out


def library_sizes(c):
    """(devit_block_acts_sizes, devit_block_bwd_sizes) of the case as dicts by buffer name (host functions: no GPU needed)"""
    from devit_amd import _lib as L
    d = dims(c)
    sa, sb = (C.c_size_t * len(ACT_NAMES))(), (C.c_size_t * len(BWD_NAMES))()
    L.call("devit_block_acts_sizes", d["B"], d["N"], d["D"], d["Da"], d["Hd"], c["flags"], sa)
    L.call("devit_block_bwd_sizes", d["B"], d["N"], d["D"], d["Da"], d["Hd"], sb)
    return dict(zip(ACT_NAMES, sa)), dict(zip(BWD_NAMES, sb))


# ============================================================================================ the lean last block, stage by stage
# devit_tail_fwd / devit_tail_bwd read line by line.  The branch half is the block's own code on a Ctx of T = B ntok rows with ntok rows per DropPath
# scale: branch_forward_stages / branch_backward_stages with geo = (T, pad_rows(T), ntok), route wmode = 0 (Wgrads wg(ct, nullptr, 0, ...): split-K
# launches on the caller's stream) and fc2's bias from fc2's own launch (g2_bias_done = false and no grouped launch, so no column-sum pass).
# A case is a block case (flags = DEVIT_BLK_SAVE) + ntok + its runs: (tag, environment, is a defer_jobs slot offered).
def _tail_case(name, B, N, ntok, D, heads, hidden, runs=(("", {}, False),)):
    return dict(_case(name, B, N, D, heads, hidden, SAVE), ntok=ntok, runs=runs)


TAIL_CASES = [
    # split-K for the all-rows product; the product handed out as a job (the test runs it); a slot offered under DEVIT_WGRADFR=0: not taken
    _tail_case("tail_student", 3, 198, 2, 384, 6, 1536,
               runs=(("split_k", {}, False), ("deferred", {}, True), ("wgradfr0", {"DEVIT_WGRADFR": "0"}, True))),
    _tail_case("tail_one_token", 2, 197, 1, 256, 4, 512, runs=(("", {}, True),)),      # D != 384: never deferred, even when a slot is offered
    _tail_case("tail_compacted", 3, 51, 2, 384, 4, 640),                               # attn_width 256: every Da-versus-D offset and ld differs
    _tail_case("tail_short", 4, 6, 2, 384, 6, 768),                                    # the 32-pixel geometry: fewer keys than one attention tile
    _tail_case("tail_two_tiles", 130, 6, 2, 384, 6, 768),                              # T = 260 crosses a row tile; Tp = 512; pad rows 260 .. 511
    _tail_case("tail_wide_tokens", 2, 198, 40, 384, 6, 1536),                          # several query rows per image in the rows-form backward
]
TAIL_FWD_STAGES = ("ln1", "mean1", "rstd1", "kv", "ln1_tok", "q", "attn_o", "lse", "x_tok", "x1", "ln2", "mean2", "rstd2", "h", "h_pre", "x2")
TAIL_BWD_STAGES = ("fc2_b", "fc2_w", "dh_pre", "dln2", "fc1_w", "fc1_b", "dx1", "g1", "n2w", "n2b", "proj_b", "dattn", "proj_w", "dq", "dkv", "dqkv_kv",
                   "dln1_tok", "dln1", "dln1/tok", "qkv_w/kv", "qkv_b/kv", "qkv_w/q", "qkv_b/q", "dx_in", "dx_in/tok", "n1w", "n1b")
# 16-bit buffers whose rows beyond the live ones the two calls zero: T-row buffers (the caller's g2 among them), M-row buffers
TAIL_PADDED_T = ("ln1_tok", "q", "attn_o", "ln2", "h", "h_pre", "dh_pre", "dln2", "g1", "dattn", "dqkv", "dln1_tok", "g2")
TAIL_PADDED_M = ("ln1", "kv", "dkv", "dln1")
# planted wiring bug of tail_emulate -> the stage, or the untouched-bytes statement, that must see it
TAIL_MUTATIONS = {
    "kv_weight_at_q": "dln1",                    # the K/V dgrad reads qkv_w16 without the Da * D offset
    "kv_weight_at_q_fwd": "kv",                  # the K/V forward product likewise
    "kv_bias_grad_at_q": "qkv_b/kv",             # g.qkv_b without + Da
    "dkv_token_rows_not_copied": "dqkv_kv",
    "dq_ld_Da": "qkv_w/q",                       # the Q weight gradient reads dQ at ld = Da instead of 3 Da
    "dln1_tok_not_scattered": "dln1/tok",
    "dx1_not_added": "dx_in/tok",
    "dx1_added_at_packed_rows": "dx_in",         # at rows b * ntok + t of dx_in instead of b * N + t
    "droppath_per_N_rows": "x1",                 # the scale of row r taken as r / N instead of r / ntok
    "pad_rows_left": "pad_rows/dkv",
    "g2_pad_not_zeroed": "pad_rows/g2",
    "token_q_wgrad_over_kv_too": "qkv_w/kv",     # the T-row weight gradient launched with 3 Da columns: the K/V token rows counted twice
    "deferred_and_launched": "qkv_w/kv",         # the all-rows product both handed out as a job and launched
}


def tail_case_named(name):
    return next(c for c in TAIL_CASES if c["name"] == name)


def tail_variants():
    """(id, case, environment, slot offered) of every run of the tail table"""
    return [(c["name"] + ("/" + tag if tag else ""), c, env, offered) for c in TAIL_CASES for tag, env, offered in c["runs"]]


def tail_dims(c, ntok):
    d = dims(c)
    Tr = d["B"] * ntok
    return dict(d, ntok=ntok, T=Tr, Tp=pad_rows(Tr))


def tail_routes(c, ntok, env=None, offered=False, fused=False):
    """the decisions of devit_tail_bwd: `branch` is routes() of the token-row Ctx (wmode 0, fc2's bias from its own launch; fused: what
    devit_dgrad_layernorm_bwd_fused(pad_rows(T), D, hidden) answers); kv_job: the all-rows product (dK | dV)^T ln1 is handed to the caller as a
    job of the grouped launch -- a slot offered, wgrad_mode of the ALL-rows Ctx (D == 384, three K-steps, DEVIT_WGRADFR != 0), and 2 Da a multiple of 128"""
    d = tail_dims(c, ntok)
    wmode_all = d["D"] == 384 and d["Mp"] // 64 >= 3 and (env or {}).get("DEVIT_WGRADFR", "1") != "0"
    return dict(branch=dict(wmode=False, fc2_bias="launch", fused=(bool(fused), False), prev=False),
                kv_job=bool(offered and wmode_all and (2 * d["Da"]) % 128 == 0))


def tok_rows(B, N, ntok, dev="cpu"):
    """the rows b * N + t, t < ntok, of an all-rows buffer, in the order of the packed token rows b * ntok + t"""
    return (torch.arange(B, device=dev)[:, None] * N + torch.arange(ntok, device=dev)[None, :]).reshape(-1)


def tail_inputs(c, ntok, key=0):
    """as inputs(), for the lean block: x on all M rows; dx and g2 = bf16(dp2 dx) on the T token rows (ntok rows per scale); no dqkv_add, no block
    below; acc0: what every gradient accumulator holds before the call"""
    d = tail_dims(c, ntok)
    M, Tr, D, Da, Hd = d["M"], d["T"], d["D"], d["Da"], d["Hd"]
    g = gen("tail", c["name"], "x", key)
    w = block_weights(c, key)
    x = T.randn(g, M, D) + 2 * T.randn(g, M, 1)
    dx = T.randn(g, Tr, D)
    inp = dict(w=w, x=x, dx=dx, g2=(dx * w["dp2"].repeat_interleave(ntok)[:, None]).to(BF16))
    shapes = dict(n1w=(D,), n1b=(D,), qkv_w=(3 * Da, D), qkv_b=(3 * Da,), proj_w=(D, Da), proj_b=(D,), n2w=(D,), n2b=(D,), fc1_w=(Hd, D),
                  fc1_b=(Hd,), fc2_w=(D, Hd), fc2_b=(D,))
    inp["acc0"] = {k: 3 * T.randn(g, *s) for k, s in shapes.items()}
    return inp


def tail_buffer_shapes(c, ntok):
    """name -> (rows, cols, 16-bit?) of every buffer devit_tail_fwd / devit_tail_bwd write, as the sequence addresses them ('kv' is the qkv slot)"""
    d = tail_dims(c, ntok)
    M, Mp, Tr, Tp, D, Da, Hd = d["M"], d["Mp"], d["T"], d["Tp"], d["D"], d["Da"], d["Hd"]
    return dict(ln1=(Mp, D, 1), mean1=(1, M, 0), rstd1=(1, M, 0), kv=(Mp, 2 * Da, 1), attn_o=(Tp, Da, 1), lse=(d["B"] * d["H"], ntok, 0), x1=(Tr, D, 0),
                ln2=(Tp, D, 1), mean2=(1, Tr, 0), rstd2=(1, Tr, 0), h=(Tp, Hd, 1), h_pre=(Tp, Hd, 1), x2=(Tr, D, 0), ln1_tok=(Tp, D, 1), q=(Tp, Da, 1),
                x_tok=(Tr, D, 0), dh_pre=(Tp, Hd, 1), dln2=(Tp, D, 1), dx1=(Tr, D, 0), g1=(Tp, D, 1), dattn=(Tp, Da, 1), dqkv=(Tp, 3 * Da, 1),
                dln1=(Mp, D, 1), dkv=(Mp, 2 * Da, 1), dln1_tok=(Tp, D, 1))


def _exact(name, got, want):
    """a stage that is a copy: the reference is the source's value, the bound 0 -- any difference is an infinite ratio"""
    want = want.to(F64)
    return name, got, want, torch.zeros_like(want)


def tail_forward_stages(c, ntok, inp, bufs):
    """yields (stage, got, float64 reference, bound) for what devit_tail_fwd left, read off it line by line: LN1 on all rows, (K | V) on all rows
    from the K/V rows of the weight and bias, the token rows of ln1 gathered, Q on them, the rows-form attention, the token rows of x gathered,
    then the block's branch half on the T token rows"""
    d, w = tail_dims(c, ntok), inp["w"]
    B, N, H, M, Tr, Tp, Da = d["B"], d["N"], d["H"], d["M"], d["T"], d["Tp"], d["Da"]
    x = bufs["x"]
    tok = tok_rows(B, N, ntok, x.device)
    yield from _ln_fwd_stage("1", x, w["n1w"], w["n1b"], bufs["ln1"][:M], bufs["mean1"], bufs["rstd1"], False, True)
    ref, bnd = G.statement(G.STORE_BF16, _d(bufs["ln1"][:M]), _d(w["qkv_w16"][Da:]), bias=_d(w["qkv_b"][Da:]))
    yield "kv", bufs["kv"][:M], ref["out"], bnd["out"]
    yield _exact("ln1_tok", bufs["ln1_tok"][:Tr], bufs["ln1"][tok])
    ref, bnd = G.statement(G.STORE_BF16, _d(bufs["ln1_tok"][:Tr]), _d(w["qkv_w16"][:Da]), bias=_d(w["qkv_b"][:Da]))
    yield "q", bufs["q"][:Tr], ref["out"], bnd["out"]
    q, k, v = A.heads(bufs["q"], B, ntok, H), A.heads(bufs["kv"], B, N, H, 0), A.heads(bufs["kv"], B, N, H, Da)
    r, b = A.bounds(q, k, v, w["head_gate"], 0.125)
    yield "attn_o", A.heads(bufs["attn_o"], B, ntok, H), r["O"], b["O"]
    yield "lse", bufs["lse"].view(B, H, ntok), r["lse"], b["lse"]
    yield _exact("x_tok", bufs["x_tok"], x[tok])
    yield from branch_forward_stages(c, inp, bufs, bufs["x_tok"], (Tr, Tp, ntok))


def tail_backward_stages(c, ntok, inp, bufs, route):
    """yields (stage, got, float64 reference, bound) for what devit_tail_bwd left, read off it line by line.  route: tail_routes().  The branch half
    on the token rows, then the lean block's own wiring, every stage stated on its inputs as they lie in memory:
        dq          columns [0, Da) of the [Tp][3 Da] buffer;  dkv [Mp][2 Da]: _attn_model.bounds in rows form, NQ = ntok
        dqkv_kv     columns [Da, 3 Da) of the token rows: the token rows of dkv, bit for bit
        dln1_tok    the K = 3 Da product of dqkv against qkv_w16;  dln1 off the token rows: the K = 2 Da product of dkv against qkv_w16[Da:];
        dln1/tok    the token rows of dln1: dln1_tok, bit for bit
        qkv_w/kv, qkv_b/kv   dkv^T ln1 over Mp rows into rows [Da, 3 Da): a job of the grouped launch (route['kv_job']) or split-K
        qkv_w/q, qkv_b/q     dQ^T ln1_tok over Tp rows into rows [0, Da): split-K, dQ read at ld = 3 Da
        dx_in, n1w, n1b      _tail_model.ln_bwd_bounds without a residual on the stored dln1; dx_in/tok: the token rows, where the reference is that
                             statement + the stored dx1 and the bound the statement's + U |reference| -- the add is a separate pass over a stored
                             fp32 value (devit_token_rows_copy with add = 1): one fp32 rounding of the sum, the one term that is new here"""
    d, w, a0 = tail_dims(c, ntok), inp["w"], inp["acc0"]
    B, N, H, M, Mp, Tr, Tp, Da = d["B"], d["N"], d["H"], d["M"], d["Mp"], d["T"], d["Tp"], d["Da"]
    acc = bufs["acc"]
    dev = bufs["dx"].device
    tok = tok_rows(B, N, ntok, dev)
    off = torch.ones(M, dtype=torch.bool, device=dev)
    off[tok] = False
    yield from branch_backward_stages(c, inp, bufs, route["branch"], (Tr, Tp, ntok))
    q, k, v = A.heads(bufs["q"], B, ntok, H), A.heads(bufs["kv"], B, N, H, 0), A.heads(bufs["kv"], B, N, H, Da)
    r, b = A.bounds(q, k, v, w["head_gate"], 0.125, A.heads(bufs["dattn"], B, ntok, H))
    yield "dq", A.heads(bufs["dqkv"], B, ntok, H, 0), r["dQ"], b["dQ"]
    got = torch.stack([A.heads(bufs["dkv"], B, N, H, j * Da) for j in range(2)])
    yield "dkv", got, torch.stack([r["dK"], r["dV"]]), torch.stack([b["dK"], b["dV"]])
    yield _exact("dqkv_kv", bufs["dqkv"][:Tr, Da:], bufs["dkv"][tok])
    ref, bnd = G.statement(G.STORE_BF16, _d(bufs["dqkv"][:Tr]), _d(w["qkv_w16"]).t())
    yield "dln1_tok", bufs["dln1_tok"][:Tr], ref["out"], bnd["out"]
    ref, bnd = G.statement(G.STORE_BF16, _d(bufs["dkv"][:M][off]), _d(w["qkv_w16"][Da:]).t())
    yield "dln1", bufs["dln1"][:M][off], ref["out"], bnd["out"]
    yield _exact("dln1/tok", bufs["dln1"][tok], bufs["dln1_tok"][:Tr])
    names = {"qkv_w": "qkv_w/kv", "qkv_b": "qkv_b/kv"}
    for name, ref, bnd in _wgrad_stage("qkv_w", "qkv_b", bufs["dkv"], bufs["ln1"], a0["qkv_w"][Da:], a0["qkv_b"][Da:], M, Mp, dict(wmode=route["kv_job"])):
        yield names[name], acc[name][Da:], ref, bnd
    names = {"qkv_w": "qkv_w/q", "qkv_b": "qkv_b/q"}
    for name, ref, bnd in _wgrad_stage("qkv_w", "qkv_b", bufs["dqkv"][:, :Da], bufs["ln1_tok"], a0["qkv_w"][:Da], a0["qkv_b"][:Da], Tr, Tp, dict(wmode=False)):
        yield names[name], acc[name][:Da], ref, bnd
    r, b = T.ln_bwd_bounds(bufs["x"], bufs["mean1"], bufs["rstd1"], w["n1w"], bufs["dln1"][:M], None, a0["n1w"], a0["n1b"])
    yield "dx_in", bufs["dx_in"][off], r["dx"][off], b["dx"][off]
    ref = r["dx"][tok] + _d(bufs["dx1"])
    yield "dx_in/tok", bufs["dx_in"][tok], ref, b["dx"][tok] + U * ref.abs()
    yield "n1w", acc["n1w"], r["dgamma"], b["dgamma"]
    yield "n1b", acc["n1b"], r["dbeta"], b["dbeta"]


def tail_audit(c, ntok, inp, bufs, route=None, arena=None):
    """-> ({stage: worst |err| / bound over EVERY live element}, problems).  route None: the forward alone.  problems names every untouched-bytes
    statement that does not hold: 'pad_rows/<buffer>' (rows >= T of a Tp-row 16-bit buffer, the caller's g2 among them, or rows >= M of ln1, kv,
    dkv, dln1, not zero), 'inputs/<name>' (x, dx or the first T rows of g2 did not come back bit for bit), and, with the TailArena the buffers
    were carved from, 'extent/<slot>' / 'guard/...' (a byte beyond a slot's stated extent, or of a guard slot, is no longer the prefill)"""
    d = tail_dims(c, ntok)
    M, Tr = d["M"], d["T"]
    rt = {}
    for name, got, ref, bnd in tail_forward_stages(c, ntok, inp, bufs):
        rt[name] = ratio(got, ref, bnd)
    if route is not None:
        for name, got, ref, bnd in tail_backward_stages(c, ntok, inp, bufs, route):
            rt[name] = ratio(got, ref, bnd)
    problems = []
    for names, live in ((TAIL_PADDED_T, Tr), (TAIL_PADDED_M, M)):
        for name in names:
            t = bufs.get(name)
            if t is not None and bool((t[live:].view(torch.int16) != 0).any()):
                problems.append("pad_rows/" + name)
    for name in ("x", "dx", "g2"):
        if bufs.get(name) is not None and not torch.equal(bufs[name][:inp[name].shape[0]].cpu(), inp[name].cpu()):
            problems.append("inputs/" + name)
    if arena is not None:
        problems += arena.written_outside()
    return rt, problems


ARENA_FILL, ARENA_GUARD = 0x55, 4096


class TailArena:
    """Every buffer of the two calls carved back to back out of ONE allocation at exactly the sizes devit_tail_acts_sizes / devit_tail_bwd_sizes
    report (and, 256-aligned, dx_in, the caller's g2 and the twelve accumulators), a guard slot in front and behind, every byte 0x55 before the
    call: in bf16 and in fp32 a finite 1.5e13, so a pad row left alone, an element never written and a read of junk all show.  `extents`: the bytes
    of each slot the calls may write (tail_extents(); the whole of lnws, which is the library's scratch)."""

    def __init__(self, dev, sizes, extents):
        self.sizes, self.extents, self.off, off = dict(sizes), dict(extents), {}, ARENA_GUARD
        for name, n in self.sizes.items():
            assert n % 256 == 0 and self.extents[name] <= n, (name, n, self.extents[name])
            self.off[name] = off
            off += n
        self.end = off
        self.mem = torch.full((off + ARENA_GUARD,), ARENA_FILL, dtype=torch.uint8, device=dev)

    def adr(self, name):
        return self.mem.data_ptr() + self.off[name] if self.sizes[name] else None

    def view(self, name, rows, cols, dtype):
        o = self.off[name]
        assert rows * cols * dtype.itemsize <= self.sizes[name], name
        return self.mem[o:o + rows * cols * dtype.itemsize].view(dtype).view(rows, cols)

    def refill(self, names, byte):
        for n in names:
            self.mem[self.off[n]:self.off[n] + self.sizes[n]] = byte

    def written_outside(self, fill=None):
        """-> 'extent/<slot>' for every slot with a changed byte beyond its extent, 'guard/front', 'guard/back'.  fill: {slot: byte} where a slot was
        refilled with another byte than 0x55"""
        fill = fill or {}
        bad = ["extent/" + n for n, e in self.extents.items()
               if not bool((self.mem[self.off[n] + e:self.off[n] + self.sizes[n]] == fill.get(n, ARENA_FILL)).all())]
        bad += ["guard/front"] if not bool((self.mem[:ARENA_GUARD] == ARENA_FILL).all()) else []
        return bad + (["guard/back"] if not bool((self.mem[self.end:] == ARENA_FILL).all()) else [])


def tail_arena(dev, c, ntok):
    """the TailArena of a case: the library's sizes for the 17 + 10 buffers ('kv' is the qkv slot), dx_in [M][D] fp32, g2 [Tp][D] bf16 and 'g_<name>'
    per accumulator"""
    d = tail_dims(c, ntok)
    al = lambda n: (n + 255) // 256 * 256                                                       # noqa: E731
    sa, sb = tail_library_sizes(d["B"], d["N"], ntok, d["D"], d["Da"], d["Hd"], SAVE)
    ea, eb = tail_extents(d["B"], d["N"], ntok, d["D"], d["Da"], d["Hd"], 1)
    sizes, ext = {}, {}
    for s, e in ((sa, ea), (sb, eb)):
        for n in s:
            sizes["kv" if n == "qkv" else n], ext["kv" if n == "qkv" else n] = s[n], e[n]
    ext["lnws"] = sizes["lnws"]
    acc = {"g_" + n: t.numel() * 4 for n, t in tail_inputs(c, ntok)["acc0"].items()}
    for n, e in dict(acc, dx_in=d["M"] * d["D"] * 4, g2=d["Tp"] * d["D"] * 2).items():
        sizes[n], ext[n] = al(e), e
    return TailArena(dev, sizes, ext)


def tail_emulate(c, ntok, inp, mutate=None, route=None):
    """devit_tail_fwd + devit_tail_bwd in fp32 torch, in the project's rounding (as emulate(), whose branch halves it runs on the token rows), every
    buffer as the two calls would leave it -> bufs as tail_audit() takes them.  `mutate`: one of TAIL_MUTATIONS, a planted WIRING bug of the lean
    block's own wiring -- every kernel stays correct.  route: tail_routes() (only deferred_and_launched reads it: it needs the job handed out)."""
    assert mutate is None or mutate in TAIL_MUTATIONS
    d, w, a0 = tail_dims(c, ntok), inp["w"], inp["acc0"]
    B, N, H, M, Mp, Tr, Tp, Da = d["B"], d["N"], d["H"], d["M"], d["Mp"], d["T"], d["Tp"], d["Da"]
    route = route or tail_routes(c, ntok)
    f = _f32
    pm = lambda v: _padded(v, M, Mp, BF16)                                                      # noqa: E731
    pt = lambda v: _padded(v, Tr, Tp, BF16)                                                     # noqa: E731
    st = _emu_drop_state(c, None)
    tok = tok_rows(B, N, ntok)
    x = inp["x"]
    per = N if mutate == "droppath_per_N_rows" else ntok
    dp1, dp2 = (w[n][torch.arange(Tr) // per][:, None] for n in ("dp1", "dp2"))
    bufs = dict(x=x.clone())
    e = T.ln_fwd_emulate(x, w["n1w"], w["n1b"], EPS)
    bufs.update(ln1=pm(e["y"]), mean1=e["mean"], rstd1=e["rstd"])
    kv_w = w["qkv_w16"][:2 * Da] if mutate == "kv_weight_at_q_fwd" else w["qkv_w16"][Da:]
    bufs["kv"] = pm(f(bufs["ln1"][:M]) @ f(kv_w).t() + w["qkv_b"][Da:])
    bufs["ln1_tok"] = pt(bufs["ln1"][tok])
    bufs["q"] = pt(f(bufs["ln1_tok"][:Tr]) @ f(w["qkv_w16"][:Da]).t() + w["qkv_b"][:Da])
    q, k, v = A.heads(bufs["q"], B, ntok, H), A.heads(bufs["kv"], B, N, H, 0), A.heads(bufs["kv"], B, N, H, Da)
    ae = A.emulate(q, k, v, w["head_gate"], 0.125)
    bufs["attn_o"], bufs["lse"] = pt(A.rows(ae["O"])), ae["lse"].to(F32)
    bufs["x_tok"] = x[tok].clone()
    _emu_branch_fwd(c, inp, bufs, bufs["x_tok"], (Tr, Tp, ntok), dp1, dp2, mutate, None, st)
    # ---- backward
    acc = {}
    _emu_branch_bwd(c, inp, bufs, acc, (Tr, Tp, ntok), dp1, mutate, None, st, route["branch"])
    bufs["g2"] = pt(inp["g2"])                   # the caller's buffer, pad rows and all: the call zeroes them
    if mutate == "g2_pad_not_zeroed":
        bufs["g2"][Tp - 1] = 1.5
    ae = A.emulate(q, k, v, w["head_gate"], 0.125, A.heads(bufs["dattn"], B, ntok, H))
    bufs["dkv"] = pm(torch.cat([A.rows(ae["dK"]), A.rows(ae["dV"])], 1))
    if mutate == "pad_rows_left":
        bufs["dkv"][M] = -0.75
    dqkv = torch.zeros((Tp, 3 * Da), dtype=BF16)
    dqkv[:Tr, :Da] = A.rows(ae["dQ"]).to(BF16)
    if mutate != "dkv_token_rows_not_copied":
        dqkv[:Tr, Da:] = bufs["dkv"][tok]
    bufs["dqkv"] = dqkv
    kv_w = w["qkv_w16"][:2 * Da] if mutate == "kv_weight_at_q" else w["qkv_w16"][Da:]
    bufs["dln1"] = pm(f(bufs["dkv"][:M]) @ f(kv_w))
    bufs["dln1_tok"] = pt(f(dqkv[:Tr]) @ f(w["qkv_w16"]))
    if mutate != "dln1_tok_not_scattered":
        bufs["dln1"][tok] = bufs["dln1_tok"][:Tr]
    acc["qkv_w"], acc["qkv_b"] = a0["qkv_w"].clone(), a0["qkv_b"].clone()
    times = 2 if (mutate == "deferred_and_launched" and route["kv_job"]) else 1
    acc["qkv_w"][Da:] += times * (f(bufs["dkv"]).t() @ f(bufs["ln1"]))
    b0 = 0 if mutate == "kv_bias_grad_at_q" else Da
    acc["qkv_b"][b0:b0 + 2 * Da] += times * f(bufs["dkv"]).sum(0)
    if mutate == "token_q_wgrad_over_kv_too":
        acc["qkv_w"] += f(dqkv).t() @ f(bufs["ln1_tok"])
        acc["qkv_b"] += f(dqkv).sum(0)
    else:
        dq = dqkv.reshape(-1)[:Tp * Da].view(Tp, Da) if mutate == "dq_ld_Da" else dqkv[:, :Da]
        acc["qkv_w"][:Da] += f(dq).t() @ f(bufs["ln1_tok"])
        acc["qkv_b"][:Da] += f(dq).sum(0)
    e = T.ln_bwd_emulate(x, bufs["mean1"], bufs["rstd1"], w["n1w"], bufs["dln1"][:M], None, a0["n1w"], a0["n1b"])
    bufs["dx_in"], acc["n1w"], acc["n1b"] = e["dx"], e["dgamma"], e["dbeta"]
    if mutate == "dx1_added_at_packed_rows":
        bufs["dx_in"][:Tr] += bufs["dx1"]
    elif mutate != "dx1_not_added":
        bufs["dx_in"][tok] += bufs["dx1"]
    bufs["acc"] = acc
    return bufs
