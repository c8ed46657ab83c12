"""The fused tails with a learning rate per granule on a real MI355X (csrc/optim.hip: devit_adamw_step_lrs, devit_sgd_step_lrs, devit_adam_l2_step_lrs,
devit_lamb_step_lrs): each against the float64 statements of tests/_lrscale_model.py within their elementwise bounds, three chained steps, on the
cases tests/test_lrscale_model.py holds the model itself to; an all-ones table against the unscaled entry point, bit for bit; one step of what the
CLIs build with --layer-decay against the step without it; and --resume under --deterministic --layer-decay."""
import argparse
import shutil

import pytest
import torch

import _lrscale_model as S
import _optim_model as M
from _tail_model import BF16, F32, F64, TINY, U, ratio
from conftest import chk
from test_gpu_tail import Out, call, refused, same_bits

pytestmark = pytest.mark.gpu

ENTRY = {"adamw": "devit_adamw_step", "adam": "devit_adam_l2_step", "momentum": "devit_sgd_step", "nesterov": "devit_sgd_step"}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from devit_amd import _lib
    _lib.require_device(torch.zeros(1, device="cuda"))
    return torch.device("cuda")


def _L():
    from devit_amd import _lib
    return _lib


def _report(tag, worst):
    for k, r in worst.items():
        print(f"tail/{tag}/{k} {r:.3f}")
        assert chk(r, 1.0, name=f"tail/{tag}/{k}"), (tag, k, r)


# ============================================================================================ the three grid-stride tails
def _run(dev, kind, c, lrs, hold=True):
    """three chained steps of `kind` on the case's inputs through the *_lrs entry point (lrs = (lr_group4, lr_scales), CPU) or the unscaled one
    (lrs None) -> (the outputs' bits after every step, worst ratios against the statement applied to the state the kernel left)"""
    L = _L()
    i = M.step_inputs(c)
    n, hp = c["n"], M.ADAM_HP if kind == "adamw" else M.OPT_HP
    names = ("p", "buf") if kind in ("momentum", "nesterov") else ("p", "m", "v")
    st = {k: Out(dev, 1, n, init=i["p"] if k == "p" else torch.zeros(n)) for k in names}
    if c["ema"]:
        st["ema"] = Out(dev, 1, n, init=i["p"])
    p16 = Out(dev, 1, n, BF16) if c["p16"] else None
    mask = None if i["mask"] is None else i["mask"].to(dev)
    nws = L.load().devit_sumsq_workspace()
    ws, gsq = torch.empty(nws, dtype=torch.uint8, device=dev), torch.empty(1, device=dev)
    extra = () if lrs is None else (lrs[0].to(dev), lrs[1].to(dev))
    worst, bits = {}, []
    for step in (1, 2, 3):
        g = i["grads"][step - 1]
        gd = g.to(dev)
        before = {k: t.v[0].cpu().clone() for k, t in st.items()}
        if c["gnorm"]:
            call("devit_sumsq_f32", gd, n, gsq, ws, nws)
        ema_t, p16_t, gsq_t = st["ema"].t if c["ema"] else None, p16.t if p16 else None, gsq if c["gnorm"] else None
        if kind in ("momentum", "nesterov"):
            dyn = torch.tensor([hp["lr"]], dtype=F32, device=dev)
            args = (st["p"].t, gd, st["buf"].t, ema_t, p16_t, mask, gsq_t, dyn, n, hp["momentum"], int(kind == "nesterov"), hp["wd"], c["max_norm"],
                    hp["ema_decay"], c["grad_scale"])
        else:
            dyn = torch.tensor([hp["lr"], 1 - hp["beta1"] ** step, 1 - hp["beta2"] ** step], dtype=F32, device=dev)
            args = (st["p"].t, gd, st["m"].t, st["v"].t, ema_t, p16_t, mask, gsq_t, dyn, n, hp["beta1"], hp["beta2"], hp["eps"], hp["wd"],
                    c["max_norm"], hp["ema_decay"], c["grad_scale"])
        call(ENTRY[kind] + ("_lrs" if lrs else ""), *args, *extra)
        assert all(t.intact() for t in st.values()) and (p16 is None or p16.intact())
        if p16:
            assert same_bits(p16.v, st["p"].v.to(BF16)), "p_bf16 == bf16(p)"
        if hold:
            state = (before["buf"],) if "buf" in before else (before["m"], before["v"])
            ref, bnd = S.step_bounds(kind, lrs[0], torch.nan_to_num(lrs[1], nan=1.0), before["p"], g, state, before.get("ema"), i["mask"],
                                     gsq.cpu() if c["gnorm"] else None, step, c["max_norm"], c["grad_scale"])
            assert set(ref) == set(st)
            for k in ref:
                worst[k] = max(worst.get(k, 0.0), ratio(st[k].v[0], ref[k], bnd[k]))
        bits.append({k: t.v[0].cpu().clone() for k, t in st.items()})
        if p16:
            bits[-1]["p16"] = p16.v[0].cpu().clone()
    return bits, worst


@pytest.mark.parametrize("kind", S.KINDS)
@pytest.mark.parametrize("c", S.step_cases(), ids=S.case_id)
def test_lrs_steps(dev, c, kind):
    """every entry of the table that no group uses holds NaN: a granule that read another entry than its own shows as NaN in p"""
    group4, table = S.group_arrays(c, fill=float("nan"))
    bits, worst = _run(dev, kind, c, (group4, table))
    _report(f"{kind}_step_lrs/{S.case_id(c)}", worst)
    grp = S.element_groups(group4)
    if 0.0 in c["scales"]:          # a scale of 0 freezes the learning rate (AdamW's decay is by lr wd: 0 too): nothing moves ...
        frozen = grp == c["bytes"][c["scales"].index(0.0)]
        assert torch.equal(bits[-1]["p"][frozen], M.step_inputs(c)["p"][frozen])
        assert bool((bits[-1]["m" if "m" in bits[-1] else "buf"][frozen] != 0).any()), "... and the moments still do"


@pytest.mark.parametrize("kind", S.KINDS)
def test_ones_table_gives_the_unscaled_bits(dev, kind):
    """lr * 1.0f is exact: with every table entry 1 (and arbitrary group bytes) the *_lrs entry point leaves the bits of its sibling, step after step"""
    for c in S.step_cases()[1:]:
        g = torch.Generator().manual_seed(3)
        group4 = torch.randint(0, 256, (c["n"] // 4,), generator=g).to(torch.uint8)
        plain, _ = _run(dev, kind, c, None, hold=False)
        scaled, _ = _run(dev, kind, c, (group4, torch.ones(S.TABLE)), hold=False)
        for step, (a, b) in enumerate(zip(plain, scaled), 1):
            assert set(a) == set(b)
            for k in a:
                assert same_bits(a[k], b[k]), f"{kind} {S.case_id(c)}: {k} differs from the unscaled entry point's at step {step}"


def test_lrs_refusals(dev):
    t = torch.zeros(1024, device=dev)
    b = torch.zeros(256, dtype=torch.uint8, device=dev)
    adam = lambda name, n, grp, tab: (name, t, t, t, t, None, None, None, None, t, n, 0.9, 0.999, 1e-8, 0.0, 0.0, 0.0, 1.0, grp, tab)
    sgd = lambda n, grp, tab: ("devit_sgd_step_lrs", t, t, t, None, None, None, None, t, n, 0.9, 0, 0.0, 0.0, 0.0, 1.0, grp, tab)
    for name in ("devit_adamw_step_lrs", "devit_adam_l2_step_lrs"):
        refused(*adam(name, 8, None, t))
        refused(*adam(name, 8, b, None))
        refused(*adam(name, 6, b, t))
    refused(*sgd(8, None, t))
    refused(*sgd(8, b, None))
    chunks = torch.tensor([[0, 2, 0, 0]], dtype=torch.int32, device=dev)
    lamb = lambda grp, tab: ("devit_lamb_step_lrs", t, t, t, t, None, None, t, t, 8, chunks, 1, 1, 0, 0.9, 0.999, 1e-8, 0.0, 0.0, 0.0, 1.0, t, 4096, grp, tab)
    refused(*lamb(None, t))
    refused(*lamb(b, None))


# ============================================================================================ devit_lamb_step_lrs
def _lid(c):
    return f"{'lambc' if c['trust_clip'] else 'lamb'}-par{c['exempt_parity']}-mn{c['max_norm']}-gs{c['grad_scale']}"


def _lamb_run(dev, c, i, table, lrs, hold=True):
    L = _L()
    n, hp, nseg = i["n"], M.OPT_HP, len(i["layout"])
    st = dict(p=Out(dev, 1, n, init=i["p"]), m=Out(dev, 1, n, init=i["m"]), v=Out(dev, 1, n, init=i["v"]))
    if c["ema"]:
        st["ema"] = Out(dev, 1, n, init=i["p"])
    p16 = Out(dev, 1, n, BF16, init=torch.full((n,), M.GAP))
    nch = table.shape[0]
    nlw = L.load().devit_lamb_workspace(nch, nseg)
    lws, chunks = Out(dev, 1, nlw // 4), table.to(dev)
    nws = L.load().devit_sumsq_workspace()
    ws, gsq = torch.empty(nws, dtype=torch.uint8, device=dev), torch.empty(1, device=dev)
    extra = () if lrs is None else (lrs[0].to(dev), lrs[1].to(dev))
    covered = torch.zeros(n, dtype=torch.bool)
    for o, numel, _ in i["layout"]:
        covered[o:o + numel] = True
    worst, bits = {}, []
    for step in (1, 2, 3):
        g = i["grads"][step - 1]
        gd = g.to(dev)
        before = {k: t.v[0].cpu().clone() for k, t in st.items()}
        call("devit_sumsq_f32", gd, n, gsq, ws, nws)
        dyn = torch.tensor([hp["lr"], 1 - hp["beta1"] ** step, 1 - hp["beta2"] ** step], dtype=F32, device=dev)
        call("devit_lamb_step" + ("_lrs" if lrs else ""), st["p"].t, gd, st["m"].t, st["v"].t, st["ema"].t if c["ema"] else None, p16.t, gsq, dyn, n,
             chunks, nch, nseg, int(c["trust_clip"]), hp["beta1"], hp["beta2"], hp["eps"], hp["wd"], c["max_norm"], hp["ema_decay"], c["grad_scale"],
             lws.t, nlw, *extra)
        got = {k: t.v[0] for k, t in st.items()}
        got["trust"] = lws.v[0, 2 * nch:]
        assert lws.intact() and p16.intact() and all(t.intact() for t in st.values())
        pc = st["p"].v[0].cpu()
        assert same_bits(p16.v[0].cpu()[covered], pc[covered].to(BF16)), "p_bf16 == bf16(p) on every tensor"
        assert bool((p16.v[0].cpu()[~covered].float() == M.GAP).all()) and bool((pc[~covered] == M.GAP).all()), "the padding belongs to no chunk"
        if hold:
            ref, bnd = S.lamb_step_bounds(S.LAMB_SCALES, before["p"], g, before["m"], before["v"], before.get("ema"), i["layout"], gsq.cpu(), step,
                                          c["max_norm"], c["grad_scale"], c["trust_clip"])
            assert set(ref) == set(got)
            for k in ref:
                worst[k] = max(worst.get(k, 0.0), ratio(got[k], ref[k], bnd[k]))
        bits.append({k: t.cpu().clone() for k, t in got.items()})
        bits[-1]["p16"] = p16.v[0].cpu().clone()
    return bits, worst


@pytest.mark.parametrize("c", M.lamb_cases(), ids=_lid)
def test_lamb_step_lrs(dev, c):
    """_optim_model.LAMB_SIZES with its padding gaps, one group per tensor (_lrscale_model.LAMB_BYTES / LAMB_SCALES; unused table entries NaN); the
    trust ratios of step 1 are the unscaled entry point's, bit for bit: neither the moments nor the norms see the scale"""
    from devit_amd import optim
    i = M.lamb_inputs(c)
    sizes, offsets = [s for _, s, _ in i["layout"]], [o for o, _, _ in i["layout"]]
    names = [f"t{s}" for s in range(len(sizes))]
    table = optim.validate_chunk_table(optim.lamb_chunk_table(names, sizes, offsets, {nm for nm, (_, _, ex) in zip(names, i["layout"]) if ex}),
                                       sizes, offsets, i["n"])
    group4, scales = S.lamb_group_arrays(i["layout"], i["n"], fill=float("nan"))
    bits, worst = _lamb_run(dev, c, i, table, (group4, scales))
    _report(f"lamb_step_lrs/{_lid(c)}", worst)
    plain, _ = _lamb_run(dev, c, i, table, None, hold=False)
    assert same_bits(bits[0]["trust"], plain[0]["trust"]) and same_bits(bits[0]["m"], plain[0]["m"]) and same_bits(bits[0]["v"], plain[0]["v"])
    o, numel, _ = i["layout"][S.LAMB_SCALES.index(0.0)]
    assert torch.equal(bits[-1]["p"][o:o + numel], i["p"][o:o + numel]), "the tensor of scale 0 has not moved"
    ones, _ = _lamb_run(dev, c, i, table, (group4, torch.ones(S.TABLE)), hold=False)
    for step, (a, b) in enumerate(zip(plain, ones), 1):
        for k in a:
            assert same_bits(a[k], b[k]), f"{k} differs from the unscaled entry point's at step {step} under a table of ones"


# ============================================================================================ what the CLIs build
def _cli_args(*extra):
    import distill_sub
    args = argparse.ArgumentParser(parents=[distill_sub.get_args_parser()]).parse_args(["--opt", "adamw", "--weight-decay", "0", "--clip-grad", "0", *extra])
    distill_sub.check_supported(args)
    return args


@pytest.mark.parametrize("compacted", [False, True], ids=["dense", "compacted"])
def test_layer_decay_end_to_end(dev, compacted):
    """Two identical two-block dedeit (32 pixels, 5 classes, batch 4), the optimizers create_flat_optimizer builds from `--opt adamw --weight-decay 0
    --clip-grad 0` with and without `--layer-decay 0.5`, one real backward each (the second model then takes the first one's gradient bits, so
    that both steps start from the same numbers), one step each.  Per element, with s the fp32 scale of its tensor's layer:

        step 1 from zero moments, no decay, no clip:  p' = fl(p - q),  q = fl(fl(fl(lr s) / bc1) m' / denom),  m' and denom the same in both runs.
        q_s against s q: fl(lr s) one rounding, then in either run the division by bc1 (2), the product with m' (1) and the quotient (2):
        |q_s - s q| <= (1 + 2 * 5) u s |q| + 3 TINY (an intermediate of the scaled run below the normal range).
        The stored p': |fl(p - q) - (p - q)| <= u |p'| in either run, and dp = p' - p is exact in float64.
        |dp_decay - s dp_plain| <= u |p'_decay| + s u |p'_plain| + 11 u s |q| + 3 TINY,  |q| <= |dp_plain| + u |p'_plain|.

    The head (layer 3 of 3, scale 1) takes the plain step's bits; patch_embed.proj.weight (layer 0) moves by 0.5^3 = 1/8 of the plain step within
    that bound.  compacted: both models are compacted for training (shrink.compact(trainable=True)) between the backward and the step -- the
    masters stay the parameters of the flat buffer under their names (shrink.attach_training), so the scales built before reach them unchanged."""
    import devit_amd
    from devit_amd import ddp, optim, shrink
    torch.manual_seed(21)
    state, models, flats, opts = None, [], [], []
    x = torch.randn(4, 3, 32, 32, generator=torch.Generator().manual_seed(5)).to(dev)
    y = torch.tensor([0, 3, 1, 4], device=dev)
    for extra in (("--layer-decay", "0.5"), ()):
        model = devit_amd.create_model("dedeit", depth=2, img_size=32, num_classes=5, drop_path_rate=0.0)
        state = state or {k: v.clone() for k, v in model.state_dict().items()}
        model.load_state_dict(state)
        model.to(dev).train()
        flat = ddp.FlatParams(model).attach_bf16(model)
        args = _cli_args(*extra)
        args.lr = 1e-3
        opts.append(optim.create_flat_optimizer(args, flat, model))
        opts[-1].zero_grad()
        out = model(x)
        assert isinstance(out, (tuple, list)) and len(out) == 2          # the class head's and the distillation head's logits: both get a gradient
        sum(torch.nn.functional.cross_entropy(o.float(), y) for o in out).backward()
        if compacted:          # after the backward: the gradients below are the dense model's, the step is the compacted model's
            names = list(flat.names)
            g = torch.Generator().manual_seed(5)
            for blk in model.blocks:
                hm, nm = torch.ones(6), torch.ones(1536)
                hm[torch.randperm(6, generator=g)[:2]] = 0
                nm[torch.randperm(1536, generator=g)[:461]] = 0
                blk.attn.gate, blk.mlp.gate = hm, nm
            shrink.compact(model, trainable=True)
            assert all(blk._compact["trainable"] for blk in model.blocks)
            named = dict(model.named_parameters())
            assert flat.names == names and all(named[n] is p and p.data_ptr() == flat.flat[o:].data_ptr() and p.grad.data_ptr() == flat.flat_grad[o:].data_ptr()
                                               for n, p, o in zip(flat.names, flat.params, flat.offsets))
        models.append(model)
        flats.append(flat)
    (fd, fp), (od, op) = flats, opts
    assert od.lr_scales is not None and od.layer_decay == 0.5 and op.lr_scales is None and fd.names == fp.names and fd.offsets == fp.offsets
    assert torch.equal(fd.flat, fp.flat) and float(fd.flat_grad.abs().max()) > 0
    fp.flat_grad.copy_(fd.flat_grad)
    p0 = fd.flat.double().cpu()
    od.step()
    op.step()
    torch.cuda.synchronize()
    pd, pp = fd.flat.double().cpu(), fp.flat.double().cpu()
    scales = optim.layer_decay_scales(fd.names, 2, 0.5)
    assert scales["head.weight"] == 1.0 and scales["patch_embed.proj.weight"] == 0.125 and scales["blocks.1.attn.qkv.weight"] == 0.5
    worst = 0.0
    for name, p, o in zip(fd.names, fd.params, fd.offsets):
        sl, s = slice(o, o + p.numel()), scales[name]
        dd, dpl = pd[sl] - p0[sl], pp[sl] - p0[sl]
        q = dpl.abs() + U * pp[sl].abs()
        bound = U * pd[sl].abs() + s * U * pp[sl].abs() + 11 * U * s * q + 3 * TINY
        r = ratio(dd, s * dpl, bound)
        worst = max(worst, r)
        assert r <= 1.0, (name, s, r)
        assert float(dpl.abs().max()) > 0, name
        if s == 1.0:
            assert torch.equal(fd.flat[sl], fp.flat[sl]), f"{name}: scale 1 is the plain step"
    print(f"tail/layer_decay_e2e/{'compacted' if compacted else 'dense'}/dp {worst:.3f}")
    assert all(same_bits(fd.flat16[o:o + p.numel()], fd.flat[o:o + p.numel()].to(BF16)) for p, o in zip(fd.params, fd.offsets)), "the bf16 copy follows"


# ============================================================================================ --resume under --deterministic
def test_resume_with_layer_decay(dev, tmp_path):
    """tests/test_gpu_resume.py's pattern at its common configuration (three epochs of three steps at 64 pixels, batch 4) with --layer-decay 0.75:
    two uninterrupted runs agree (the control), and a run resumed from the first one's epoch-0 checkpoint reproduces its later checkpoints and
    log lines bit for bit.  The checkpoints carry the flag, not the scales; a resume under another value is refused with both named."""
    import distill_sub
    from test_gpu_resume import COMMON, check_continuation, uninterrupted
    flags = COMMON + ["--layer-decay", "0.75"]
    A = uninterrupted(flags, tmp_path)
    try:
        B = check_continuation(A, flags, tmp_path)
        for run in (A, B):
            sd = run.checkpoint(2)["optimizer"]
            assert sd["layer_decay"] == 0.75 and set(sd) == {"m", "v", "ema", "step", "lr", "layer_decay"}
        with pytest.raises(ValueError, match="--layer-decay 0.75 cannot be loaded into --layer-decay 0.5"):
            distill_sub.main(argparse.ArgumentParser(parents=[distill_sub.get_args_parser()]).parse_args(
                COMMON + ["--layer-decay", "0.5", "--resume", A.path(0), "--output_dir", str(tmp_path / "c")]))
    finally:
        shutil.rmtree(str(tmp_path), ignore_errors=True)
