"""Deterministic mode on a real MI355X (ops.deterministic()).  Per site -- the split-K 128 x 128 GEMM and its fused row sums,
devit_wgrad_grouped and a_colsum, devit_embed_bwd, the column sums of devit_dropout_apply, the three scalars of devit_cls_distill_loss -- on
non-integer random operands with at least three partial sums per address:
    (a) the same call five times gives torch.equal results;
    (b) fold-then-add: the call into a zeroed destination gives R, the call into a destination that holds random X gives fp32(X + R), bit for bit
        (arrival-order atomics and a fixed-order chain ((X + p_0) + p_1) + ... both fail this on random data);
    (c) the results stay inside the per-element float64 bounds the project already has for the entry point (tests/_gemm_model.py, _tail_model.py,
        _drop_model.py, imported, not edited; devit_embed_bwd has no row there: (n + 1) 2^-24 sum |terms| for its n fp32 additions);
    (d) with the mode off the same calls still meet (c).
devit_embed_bwd and devit_cls_distill_loss zero their destination themselves (accumulate is refused / the launcher's memset): for them (b) is
"a destination that holds random X gives R".  devit_embed_bwd starts one batch slice below B = 64, so the issue's B = 24 has one term per address; B = 64
(eight slices) is the case that reaches the new kernel.
Then the step: DEKD (dedeit under DeiT-B, both depth 2, B = 4, 224 and 64 pixels) forward + backward + three fused AdamW steps with EMA on two fresh
models from one state, its variants, a D = 768 model, the ensemble step, and deterministic against default mode."""
import ctypes as C

import pytest
import torch

import _drop_model as DM
import _gemm_model as G
import _imgsize_model as IM
import _tail_model as T
from conftest import chk
from oracle.detgen import det_array, det_labels

pytestmark = pytest.mark.gpu
F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
U = 2.0 ** -24


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from devit_amd import _lib
    _lib.require_device(torch.zeros(1, device="cuda"))
    return torch.device("cuda")


def hold(tag, r):
    print(f"det/{tag} {r:.4f}")
    assert chk(r, 1.0, name=f"det/{tag}"), f"det/{tag}: worst |err| / bound {r:.4f}"


def modes():
    """(name, context) of the two modes, deterministic first"""
    from devit_amd import ops
    return (("det", ops.deterministic(True)), ("default", ops.deterministic(False)))


def same(a, b):
    return all(torch.equal(a[k], b[k]) for k in a)


# ============================================================================================ the split-K GEMM on 128 x 128 tiles
def _gcase(M, N, sk, aux, **kw):
    name = f"det/kmAB/M{M}_N{N}/split{sk}{'_aux' if aux else ''}" + "".join(f"/{k}{v}" for k, v in kw.items())
    return G._case(name, G.TILE128, M, N, 768, G.ATOMIC, a_km=1, b_km=1, split_k=sk, aux=aux, **kw)


GEMM_CASES = [_gcase(M, N, sk, aux) for M, N in ((128, 128), (256, 384)) for sk in (3, 4) for aux in (False, True)] + \
    [_gcase(256, 384, 3, True, a_group=4, a_skip=2), _gcase(256, 384, 4, True, m_valid=130)]


def run_gemm(c, inp, out_init, aux_init):
    from devit_amd import ops
    got = {"out": out_init.clone()}
    if aux_init is not None:
        got["aux"] = aux_init.clone()
    args, kw = G.call_args(c, inp, lambda name, off: (got[name] if name in got else inp["bufs"][name])[off:])
    assert ops.gemm_route(*args, **kw) == G.TILE128
    ops.gemm(*args, **kw)
    torch.cuda.synchronize()
    return got


@pytest.mark.parametrize("c", GEMM_CASES, ids=[c["name"] for c in GEMM_CASES])
def test_gemm_split_k(dev, c):
    inp = G.to_device(G.inputs(c), dev)
    bufs, m_lim = inp["bufs"], inp["geo"]["m_lim"]
    live = G.live_index(c, inp["geo"]).to(dev).reshape(-1)
    out_x, aux_x = bufs["out0"], bufs.get("aux0")                      # the model's preloaded accumulators: random, non-integer
    out_z, aux_z = out_x.clone(), None if aux_x is None else aux_x.clone()
    out_z[live] = 0.0
    if aux_z is not None:
        aux_z[:m_lim] = 0.0
    ref_bnd = G.reference(c, inp)
    for mode, ctx in modes():
        with ctx:
            runs = [run_gemm(c, inp, out_x, aux_x) for _ in range(5 if mode == "det" else 1)]
            zero = run_gemm(c, inp, out_z, aux_z)
        rt, untouched = G.verdict(c, inp, runs[0], ref_bnd)                                                         # (c) / (d)
        assert untouched, f"{c['name']} ({mode}): a write outside what the call describes"
        for name, r in rt.items():
            hold(f"gemm/{c['name']}/{mode}/{name}", r)
        fold_add = torch.equal(runs[0]["out"][live], out_x[live] + zero["out"][live]) and \
            (aux_x is None or torch.equal(runs[0]["aux"][:m_lim], aux_x[:m_lim] + zero["aux"][:m_lim]))
        print(f"det/gemm/{c['name']}/{mode}: out == X + R bit for bit: {fold_add}")
        if mode == "det":
            assert all(same(runs[0], r) for r in runs[1:]), f"{c['name']}: five runs of one call differ"             # (a)
            assert fold_add, f"{c['name']}: the result into a preloaded destination is not fp32(X + R)"              # (b)


# ============================================================================================ devit_wgrad_grouped
WG_K, WG_SPLIT = 576, 3
WG_JOBS = [G._wjob("half", 128, colsum=True), G._wjob("wide_t", 384, transposed=1, colsum=False)]


def run_wgrad(ds, inits):
    from devit_amd import _lib as L, ops
    gots, structs = [], []
    for d, init in zip(ds, inits):
        got = {k: v.clone() for k, v in init.items()}
        structs.append(L.WgradJob(d["a"].data_ptr(), d["lda"], d["job"]["a_cols"], d["b"].data_ptr(), d["ldb"], got["out"].data_ptr(), d["ldc"],
                                  d["job"]["transposed"], got["colsum"].data_ptr() if "colsum" in got else None))
        gots.append(got)
    ops.call("devit_wgrad_grouped", (L.WgradJob * len(structs))(*structs), len(structs), WG_K, WG_SPLIT, L.stream_ptr())
    torch.cuda.synchronize()
    return gots


def test_wgrad_grouped(dev):
    ds = [{k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in d.items()} for d in G.wgrad_inputs("det", WG_K, WG_JOBS)]
    x_init, z_init = [], []
    for d in ds:
        x = {"out": d["out0"]}
        z = {"out": d["out0"].clone()}
        z["out"][:d["orows"] * d["ldc"]].view(d["orows"], d["ldc"])[:, :d["ocols"]] = 0.0
        if "colsum0" in d:
            x["colsum"], z["colsum"] = d["colsum0"], d["colsum0"].clone()
            z["colsum"][:d["job"]["a_cols"]] = 0.0
        x_init.append(x)
        z_init.append(z)
    for mode, ctx in modes():
        with ctx:
            runs = [run_wgrad(ds, x_init) for _ in range(5 if mode == "det" else 1)]
            zero = run_wgrad(ds, z_init)
        fold_add = True
        for d, got, x, z in zip(ds, runs[0], x_init, zero):
            rt, untouched = G.wgrad_verdict(d, got, G.wgrad_reference(d, WG_K, WG_SPLIT))
            assert untouched, f"wgrad/{d['job']['name']} ({mode}): a write outside the accumulator"
            for k, r in rt.items():
                hold(f"wgrad/{d['job']['name']}/{mode}/{k}", r)
            live = {"out": lambda v, d=d: v[:d["orows"] * d["ldc"]].view(d["orows"], d["ldc"])[:, :d["ocols"]],
                    "colsum": lambda v, d=d: v[:d["job"]["a_cols"]]}
            fold_add &= all(torch.equal(live[k](got[k]), live[k](x[k]) + live[k](z[k])) for k in got)
        print(f"det/wgrad/{mode}: out == X + R bit for bit: {fold_add}")
        if mode == "det":
            assert all(same(a, b) for r in runs[1:] for a, b in zip(runs[0], r)), "five runs of one call differ"
            assert fold_add, "the result into preloaded accumulators is not fp32(X + R)"


# ============================================================================================ devit_embed_bwd
@pytest.mark.parametrize("with16", [False, True])
@pytest.mark.parametrize("B", [24, 64])
def test_embed_bwd(dev, B, with16):
    from devit_amd import _lib as L
    Tk, D, ntok = 6, 64, 2
    g = T.gen("det/embed_bwd", B)
    dx_c = T.randn(g, B, Tk, D)
    dx, X = dx_c.to(dev), T.randn(g, Tk, D).to(dev)
    slices = 8 if B >= 64 else 1                         # (elementwise.hip: devit_embed_bwd)
    n_adds = -(-B // slices) + slices
    ref = dx_c.to(F64).sum(0)
    bnd = (n_adds + 1) * U * dx_c.to(F64).abs().sum(0)

    def run(dpos0):
        o = dict(dpos=dpos0.clone(), dcls=torch.zeros(D, device=dev), ddist=torch.zeros(D, device=dev), dbias=torch.zeros(D, device=dev))
        if with16:
            o["d16"] = torch.zeros(B * Tk, D, dtype=BF16, device=dev)
        L.call("devit_embed_bwd", L.ptr(dx), B, Tk, D, ntok, L.ptr(o["dpos"]), L.ptr(o["dcls"]), L.ptr(o["ddist"]), L.ptr(o["dbias"]),
               L.ptr(o.get("d16")), 0, L.stream_ptr())
        torch.cuda.synchronize()
        return o
    for mode, ctx in modes():
        with ctx:
            runs = [run(X) for _ in range(5 if mode == "det" else 1)]
            zero = run(torch.zeros_like(X))
        hold(f"embed_bwd/B{B}_16{int(with16)}/{mode}/dpos", T.ratio(runs[0]["dpos"], ref, bnd))
        hold(f"embed_bwd/B{B}_16{int(with16)}/{mode}/dbias", T.ratio(runs[0]["dbias"], ref[ntok:].sum(0), bnd[ntok:].sum(0) + (Tk - ntok + 1) * U * ref[ntok:].abs().sum(0)))
        assert torch.equal(runs[0]["dcls"], runs[0]["dpos"][0]) and torch.equal(runs[0]["ddist"], runs[0]["dpos"][1])
        if with16:
            assert torch.equal(runs[0]["d16"].view(torch.int16), dx.view(B * Tk, D).to(BF16).view(torch.int16))
        if mode == "det":
            assert all(same(runs[0], r) for r in runs[1:]), "five runs of one call differ"
            assert same(runs[0], zero), "the entry point zeroes dpos itself: what it held before must not matter"


# ============================================================================================ devit_dropout_apply: the column sums
DROP_CASES = [DM._a("det-bf16-9x384", BF16, 9, 384), DM._a("det-f32-9x384", F32, 9, 384, p=0.5), DM._a("det-bf16-1029x384", BF16, 1029, 384)]


@pytest.mark.parametrize("c", DROP_CASES, ids=[c["name"] for c in DROP_CASES])
def test_dropout_column_sums(dev, c):
    from devit_amd._lib import call, ptr, stream_ptr
    assert DM.grid(c)["gy"] >= 3 and (c["rows"] != 9 or (DM.grid(c)["gy"] == 3 and DM.grid(dict(c, rows=8))["gy"] == 2)), "three row strips at least"
    inp = DM.inputs(c)
    thr, s = DM.thr_s(c["p"])
    X = inp["colsum0"].to(dev)

    def run(colsum0):
        x, colsum = inp["x"].to(dev), colsum0.clone()
        call("devit_dropout_apply", ptr(x), 1 if c["dtype"] == F32 else 0, c["rows"], c["cols"], c["ld"], c["pitch"], c["seed"], c["site"], c["block"],
             thr, s, ptr(colsum), stream_ptr())
        torch.cuda.synchronize()
        return dict(x=x, colsum=colsum)
    for mode, ctx in modes():
        with ctx:
            runs = [run(X) for _ in range(5 if mode == "det" else 1)]
            zero = run(torch.zeros_like(X))
        for k, r in DM.judge_apply(c, inp, runs[0]["x"].cpu(), runs[0]["colsum"].cpu()).items():
            hold(f"dropout/{c['name']}/{mode}/{k}", r)
        fold_add = torch.equal(runs[0]["colsum"], X + zero["colsum"])
        print(f"det/dropout/{c['name']}/{mode}: colsum == X + R bit for bit: {fold_add}")
        if mode == "det":
            assert all(same(runs[0], r) for r in runs[1:]), "five runs of one call differ"
            assert fold_add, "the column sums into a preloaded destination are not fp32(X + R)"


# ============================================================================================ devit_cls_distill_loss
@pytest.mark.parametrize("kind", [0, 1, 2])
def test_cls_loss_scalars(dev, kind):
    from devit_amd import _lib as L
    B, Cn, alpha, tau = 48, 25, 0.5, (3.0 if kind == 1 else 1.0)                      # three workgroups of 16 rows
    i = T.cls_inputs(B, Cn, "std3")
    ref, bnd = T.cls_bounds(i["lo"], i["lk"], i["lt"], i["y"], kind, alpha, tau)
    lo, lk, lt, y = (i[k].to(dev) for k in ("lo", "lk", "lt", "y"))

    def run(fill):
        o = dict(loss3=torch.full((3,), fill, device=dev), dlo=torch.zeros(B, Cn, device=dev), dlk=torch.zeros(B, Cn, device=dev))
        L.call("devit_cls_distill_loss", L.ptr(lo), L.ptr(lk), L.ptr(lt), L.ptr(y), B, Cn, kind, C.c_float(alpha), C.c_float(tau), L.ptr(o["loss3"]),
               L.ptr(o["dlo"]), L.ptr(o["dlk"]), L.stream_ptr())
        torch.cuda.synchronize()
        return o
    for mode, ctx in modes():
        with ctx:
            runs = [run(7.25) for _ in range(5 if mode == "det" else 1)]
        for k in ("loss3", "dlo", "dlk"):
            hold(f"cls_loss/kind{kind}/{mode}/{k}", T.ratio(runs[0][k], ref[k], bnd[k]))
        if mode == "det":
            assert all(same(runs[0], r) for r in runs[1:]), "five runs of one call differ"


# ============================================================================================ the step
NCLS, STEP_B = 25, 4
TEACHER = "deit_base_distilled_patch16_224"
HP = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.05, max_norm=1.0, ema_decay=0.999)
_states = {}


def student(dev, S, **kw):
    """a fresh depth-2 `dedeit` at S pixels on the state every model of that key starts from"""
    import devit_amd
    key = ("dedeit", S, tuple(sorted(kw.items())))
    m = devit_amd.create_model("dedeit", num_classes=NCLS, img_size=S, depth=2, drop_path_rate=0.1, **kw)
    if key not in _states:
        torch.manual_seed(1234 + S)
        _states[key] = {k: (v.clone().normal_(0, 0.05) if v.dtype.is_floating_point and "norm" not in k else v.clone()) for k, v in m.state_dict().items()}
    m.load_state_dict(_states[key])
    return m.to(dev).train()


def teacher(dev, S):
    import devit_amd
    key = (TEACHER, S)
    if key not in _states:
        torch.manual_seed(99 + S)
        t = devit_amd.create_model(TEACHER, num_classes=NCLS, img_size=S, depth=2)
        t.load_state_dict({k: (v.clone().normal_(0, 0.05) if v.dtype.is_floating_point and "norm" not in k else v) for k, v in t.state_dict().items()})
        t.to(dev).eval()
        for p in t.parameters():
            p.requires_grad_(False)
        _states[key] = t
    return _states[key]


def batch(dev, S, tag="det/step", B=STEP_B):
    img = torch.from_numpy(det_array(f"{tag}/img{S}", (B, 3, S, S))).to(dev)
    y1, y2 = det_labels(f"{tag}/y1", B, NCLS), det_labels(f"{tag}/y2", B, NCLS)
    oh = lambda y: torch.full((B, NCLS), 0.1 / NCLS).scatter_(1, torch.from_numpy(y)[:, None], 1 - 0.1 + 0.1 / NCLS)      # noqa: E731
    dps = [(a.to(dev).contiguous(), b.to(dev).contiguous()) for a, b in IM.dp_scales_for(f"{tag}/{S}", B, depth=2)]
    return img, (oh(y1) * 0.7 + oh(y2) * 0.3).to(dev), dps


def launches_of(fn):
    """fn() with the library's launch observer on: -> (fn's result, the split-K launches it made, as dicts).  The observer belongs to the calling
    thread and the backward runs on autograd's: the way in is the one bench.py's instruments take -- while ops.PROFILE is a list, ops.call puts
    ops._record around every library call on whatever thread makes it."""
    from devit_amd import _lib as L, ops
    seen = []

    def note(phase, stream, i):
        name = i.name.decode()
        if phase == 0 and (name == "devit_wgrad_grouped" or (name == "devit_gemm_bf16" and i.kind == L.EPI_ATOMIC_F32)):
            seen.append(dict(name=name, M=i.M, N=i.N, K=i.K, split_k=i.split_k, njobs=i.njobs, a_cols=i.a_cols))
    record, ops._record, ops.PROFILE = ops._record, note, []
    try:
        out = fn()
    finally:
        ops._record, ops.PROFILE = record, None
    return out, seen


def dekd_backward(s, t, img, soft, dps, hid_gama=0.0, zero=True):
    from devit_amd import engine
    if zero:
        for p in s.parameters():
            p.grad = None
    out = engine.distill_forward(s, t, img, soft, gama=(0.2, 0.1, 0.3), kind="hard", alpha=0.5, tau=1.0, dp_scales=dps, hid_gama=hid_gama)
    out["loss"].backward()
    torch.cuda.synchronize()
    return {n: p.grad.detach().clone() for n, p in s.named_parameters() if p.grad is not None}


def differing(a, b):
    assert set(a) == set(b) and len(a) > 0
    return [n for n in a if not torch.equal(a[n], b[n])]


@pytest.mark.parametrize("S", [224, 64])
def test_dekd_step_twice(dev, S):
    """two fresh students from one state: every gradient, then masters / moments / EMA / the bf16 weight copy after three fused AdamW steps"""
    from devit_amd import ddp, ops, optim
    t = teacher(dev, S)
    img, soft, dps = batch(dev, S)
    ends = []
    with ops.deterministic():
        for _ in range(2):
            s = student(dev, S)
            flat = ddp.FlatParams(s).attach_bf16(s)
            reducer = ddp.BucketedGradReducer(flat).attach(s)
            opt = optim.FlatAdamW(flat, no_decay=optim.no_decay_names(s), **HP)
            grads, p0 = None, flat.flat.clone()
            for step in range(3):
                opt.zero_grad()
                g = dekd_backward(s, t, img, soft, dps, zero=False)
                grads = grads or g
                reducer.finish()
                opt.step()
            torch.cuda.synchronize()
            assert float((flat.flat - p0).abs().max()) > 0
            ends.append((grads, dict(p=flat.flat.clone(), m=opt.m.clone(), v=opt.v.clone(), ema=opt.ema.clone(), w16=flat.flat16.clone())))
    assert not differing(ends[0][0], ends[1][0])
    assert not differing(ends[0][1], ends[1][1])


VARIANTS = {"group_block": dict(env={"DEVIT_WGRAD_GROUP": "block"}), "group_all": dict(env={"DEVIT_WGRAD_GROUP": "all"}),
            "drop_rate": dict(model=dict(drop_rate=0.1)), "drop_rate_drawn": dict(model=dict(drop_rate=0.1), draw=True), "hid_gama": dict(hid_gama=0.5), "compacted": dict(compact=True),
            "accumulate": dict(accumulate=True),
            # B = 8: 1584 token rows, 28 K-steps -- the cost model of devit_wgrad_grouped gives block 0's 19 tiles four K slices (asserted below)
            "group_block_B8": dict(env={"DEVIT_WGRAD_GROUP": "block"}, B=8, split_block=3)}


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_dekd_gradients_twice(dev, monkeypatch, variant):
    from devit_amd import ops, shrink
    v = VARIANTS[variant]
    for k, val in v.get("env", {}).items():
        monkeypatch.setenv(k, val)
    S = 224
    t = teacher(dev, S)
    img, soft, dps = batch(dev, S, B=v.get("B", STEP_B))
    got = []
    with ops.deterministic():
        for _ in range(2):
            s = student(dev, S, **v.get("model", {}))
            # the step's draws come from torch's generators (--seed): the dropout seed of a forward from the CPU one, DropPath scales (variant
            # drop_rate_drawn: the model's own forward, pos_drop included) from the device's
            torch.manual_seed(4242)
            if v.get("draw"):
                dps = "draw"
            if v.get("compact"):
                g = torch.Generator().manual_seed(5)
                for blk in s.blocks:
                    hm, nm = torch.ones(6), torch.ones(1536)
                    hm[torch.randperm(6, generator=g)[:2]] = 0
                    nm[torch.randperm(1536, generator=g)[:461]] = 0
                    blk.attn.gate, blk.mlp.gate = hm, nm
                shrink.compact(s, trainable=True)
            grads, seen = launches_of(lambda: dekd_backward(s, t, img, soft, dps, hid_gama=v.get("hid_gama", 0.0)))
            if v.get("split_block"):      # the launch that holds block 0's four products ran in >= 3 K slices: its 19 tiles were ordered reductions
                block0 = [x for x in seen if x["name"] == "devit_wgrad_grouped" and x["njobs"] == 4]
                print(f"det/{variant}: split launches {seen}")
                assert block0 and all(x["split_k"] >= v["split_block"] for x in block0), seen
            if v.get("accumulate"):
                grads = dekd_backward(s, t, img, soft, dps, zero=False)          # a second backward into the same .grad
            got.append(grads)
    assert not differing(got[0], got[1])
    assert all(bool(torch.isfinite(g).all()) for g in got[0].values()) and any(float(g.abs().max()) > 0 for g in got[0].values())


def test_wide_model_step_twice(dev):
    """D = 768, depth 1: every weight gradient on the split-K 128 x 128 launches (the train_subdata.py path)"""
    import devit_amd
    from devit_amd import ops
    torch.manual_seed(77)
    st, got = None, []
    img = torch.from_numpy(det_array("det/wide/img", (STEP_B, 3, 224, 224))).to(dev)
    w = torch.from_numpy(det_array("det/wide/w", (STEP_B, NCLS), std=1.0)).to(dev)
    with ops.deterministic():
        for _ in range(2):
            m = devit_amd.create_model("deit_base_patch16_224", num_classes=NCLS, depth=1)
            st = st or {k: v.clone() for k, v in m.state_dict().items()}
            m.load_state_dict(st)
            m.to(dev).train()
            out = m(img)
            out = out["output"] if isinstance(out, dict) else out
            (out.float() * w).sum().backward()
            torch.cuda.synchronize()
            got.append({n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None})
    assert not differing(got[0], got[1])
    assert float(got[0]["blocks.0.mlp.fc1.weight"].abs().max()) > 0 and float(got[0]["patch_embed.proj.weight"].abs().max()) > 0


def test_ensemble_step_twice(dev):
    """MultiViT(2 x dedeit) + EnsMLP under a frozen depth-1 DeiT-B at 64 pixels (18 tokens) on the flat path: every gradient of both flat buffers.
    (The backbones keep their registered depth: MultiViT builds them by name.)"""
    import devit_amd
    import ensemble
    from devit_amd import ddp, engine, losses, ops, optim
    from devit_amd.ensemble_models import EnsMLP, MultiViT
    S = 64
    tch = devit_amd.create_model(TEACHER, num_classes=10, img_size=S, depth=1).to(dev).eval()
    for p in tch.parameters():
        p.requires_grad_(False)
    g = T.gen("det/ens")
    x, y = T.randn(g, STEP_B, 3, S, S).to(dev), torch.randint(0, 10, (STEP_B,), generator=g).to(dev)
    st, got = None, []
    with ops.deterministic():
        for _ in range(2):
            torch.manual_seed(7)
            multi = MultiViT("dedeit", num_div=2, drop_path=0, num_classes_list=[5, 5], img_size=S)
            ens = EnsMLP("dedeit", 10, 384, [5, 5], 768)
            st = st or ({k: v.clone() for k, v in multi.state_dict().items()}, {k: v.clone() for k, v in ens.state_dict().items()})
            multi.load_state_dict(st[0]); ens.load_state_dict(st[1])
            multi.to(dev).train(); ens.to(dev).train()
            crit = losses.EnsLoss(torch.nn.CrossEntropyLoss(), tch, "dedeit", "hard", 0.5, 1.0)
            flat, ens_flat = ddp.FlatParams(multi).attach_bf16(multi), ddp.FlatParams(ens)
            runner = ensemble.EnsStepRunner(ddp.BucketedGradReducer(flat).attach(multi), ddp.BucketedGradReducer(ens_flat))
            out = engine.ens_forward(multi, ens, crit, x, y, "hard")
            flat.zero_grad(); ens_flat.zero_grad()
            out["loss"].backward()
            runner.reducer.finish(); runner.ens_reducer.finish()
            torch.cuda.synchronize()
            got.append(dict(backbones=flat.flat_grad.clone(), ens=ens_flat.flat_grad.clone()))
    assert not differing(got[0], got[1])
    assert float(got[0]["backbones"].abs().max()) > 0 and float(got[0]["ens"].abs().max()) > 0


def contributors(name, shape, seen, B):
    """How many partial sums the step's launches add per address of parameter `name` (depth-2 `dedeit`: block 0 through devit_block_bwd, block 1 the
    lean tail of devit_tail_bwd, csrc/encoder.hip), read off the launches the library reported (`seen`):
      block 0's qkv / proj / fc1 weights and biases and its fc2 weight: the K slices of the grouped launch that holds its jobs (the one with >= 4 jobs);
      block 0's fc2 bias: a fixed-order column-sum pass, or -- if devit_block_bwd had to take the split-K launch for it -- that launch's row sums:
        counted as the largest [384 x 1536] launch's split_k * tiles_n;
      block 1: fc2 and fc1 on the token rows, one 128 x 128 split-K launch each, the bias from its fused row sums (split_k * tiles_n); proj's weight one
        [384 x 384] launch, its bias from the LayerNorm backward's fixed-order column sums; qkv rows [384:] (dK | dV) the grouped launch that holds that
        job or a [768 x 384] launch, rows [:384] a [384 x 384] launch: the larger count of the two row ranges;
      patch embedding weight: its [384 x 768] launch; its bias and cls / dist token: fixed-order sums over dpos; pos_embed: devit_embed_bwd's batch slices;
      LayerNorm parameters and the heads: fixed-order sums, one term."""
    def gemm(M, N, rowsums=False):
        return max([x["split_k"] * ((N // 128) if rowsums else 1) for x in seen if x["name"] == "devit_gemm_bf16" and (x["M"], x["N"]) == (M, N)], default=0)
    grouped = [x for x in seen if x["name"] == "devit_wgrad_grouped"]
    g_block0 = max([x["split_k"] for x in grouped if x["njobs"] >= 4], default=0)
    g_dkv = max([x["split_k"] for x in grouped if x["njobs"] != 4], default=0)       # (its own launch, or the five-job launch of DEVIT_WGRAD_GROUP=all)
    bias = name.endswith(".bias")
    if name.startswith("blocks.0.") and ("attn.qkv" in name or "attn.proj" in name or "mlp.fc1" in name or name == "blocks.0.mlp.fc2.weight"):
        # (without a grouped launch -- DEVIT_WGRADFR=0 -- the product's own 128 x 128 launch)
        return g_block0 if g_block0 else max(gemm(shape[0], shape[1] if len(shape) > 1 else 384, bias), 1)
    if name == "blocks.0.mlp.fc2.bias":
        return max(gemm(384, 1536, True), 1)
    if name.startswith("blocks.1.mlp.fc"):
        n, k = (384, 1536) if "fc2" in name else (1536, 384)
        return max(gemm(n, k, bias), 1)
    if name == "blocks.1.attn.proj.weight":
        return max(gemm(384, 384), 1)
    if name.startswith("blocks.1.attn.qkv"):
        return max(g_dkv, gemm(768, 384, bias), gemm(384, 384, bias), 1)
    if name == "patch_embed.proj.weight":
        return max(gemm(384, 768), 1)
    if name == "pos_embed":
        return 8 if B >= 64 else 1
    return 1


@pytest.mark.parametrize("B,group", [(4, "auto"), (8, "block")])
def test_mode_against_mode(dev, monkeypatch, B, group):
    """The two modes re-order one sum per address, nothing else: each parameter's gradients lie within (S + 1) 2^-24 sum |p_i| of each other, S = the
    partial sums p_i its addresses receive, and sum |p_i| is bounded by S times the parameter's largest gradient magnitude.  S is the parameter's own
    (contributors(): from the split-K launches the library reports for this very step; the slice counts are the same in both modes).  A parameter with
    one term per address (S = 1: the bound is 2 ulp-sized units of its maximum) has the same bits in both modes.  B = 8 with one grouped launch per
    block is the configuration in which block 0's weight gradients take several K slices."""
    from devit_amd import ops
    monkeypatch.setenv("DEVIT_WGRAD_GROUP", group)
    S = 224
    t = teacher(dev, S)
    img, soft, dps = batch(dev, S, B=B)
    with ops.deterministic():
        a, seen = launches_of(lambda: dekd_backward(student(dev, S), t, img, soft, dps))
    with ops.deterministic(False):
        b = dekd_backward(student(dev, S), t, img, soft, dps)
    print(f"det/mode_against_mode/B{B}_{group}: split launches {seen}")
    worst, counts = {}, {}
    for n in a:
        SL = counts[n] = contributors(n, tuple(a[n].flatten(1).shape) if a[n].dim() > 1 else tuple(a[n].shape), seen, B)
        bound = (SL + 1) * U * SL * float(a[n].abs().max())
        worst[n] = float((a[n].double() - b[n].double()).abs().max()) / bound if bound > 0 else float(not torch.equal(a[n], b[n]))
    top = max(worst, key=worst.get)
    differ = {n: (counts[n], round(worst[n], 4)) for n in a if not torch.equal(a[n], b[n])}
    print(f"det/mode_against_mode/B{B}_{group}: worst |det - default| / bound {worst[top]:.4f} at {top} (S = {counts[top]}); parameters whose bits differ "
          f"(S, share of the bound): {differ}; S per parameter: {counts}")
    assert all(counts[n] > 1 for n in differ), "a parameter with one term per address differs between the modes"
    hold(f"mode_against_mode/B{B}_{group}", worst[top])
