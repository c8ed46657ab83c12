"""--relation-layers without a GPU: the selection table of engine.resolve_relation_layers and its refusals, the command line's flag, and the CPU
helper the GPU tests measure against (tests/_rellayers_model.py) pinned to tests/_imgsize_model.distill_step at the middle pair, bit for bit."""
import argparse

import pytest
import torch

import _imgsize_model as IM
import _rellayers_model as RM
from oracle import devit_oracle as O
from oracle.detgen import det_array, det_labels

GS, GT = O.GEOMETRY["dedeit"], O.GEOMETRY["deit_base_distilled_patch16_224"]


def resolve(*a):
    from devit_amd import engine
    return engine.resolve_relation_layers(*a)


@pytest.mark.parametrize("sl,tl", [(12, 12), (12, 24), (6, 12)])
def test_selection_table(sl, tl):
    r = tl // sl
    mid = ((sl // 2 - 1, tl // 2 - 1),)                     # the reference's pair (engine.py:91-92) at every depth ratio
    assert resolve(None, sl, tl) == resolve("mid", sl, tl) == resolve(["mid"], sl, tl) == mid
    assert resolve("last", sl, tl) == ((sl - 1, tl - 1),)
    assert resolve("all", sl, tl) == tuple((s, (s + 1) * r - 1) for s in range(sl))
    assert resolve("all", sl, tl)[-1] == (sl - 1, tl - 1) and len(resolve("all", sl, tl)) == sl
    assert resolve([sl - 1, 0, 2, 0], sl, tl) == ((0, r - 1), (2, 3 * r - 1), (sl - 1, tl - 1))          # sorted, deduplicated
    assert resolve(("0", str(sl - 1)), sl, tl) == ((0, r - 1), (sl - 1, tl - 1))                        # the command line's strings
    assert resolve(iter([1]), sl, tl) == resolve(["1"], sl, tl) == ((1, 2 * r - 1),)
    assert resolve(range(sl), sl, tl) == resolve("all", sl, tl)
    for s, t in resolve("all", sl, tl):
        assert (s, t) == RM.pairs_for([s], sl, tl)[0]


def test_the_default_teacher_pairs_block_5_with_block_11():
    assert resolve("mid", 12, 24) == ((5, 11),) and resolve([0, 5, 11], 12, 24) == ((0, 1), (5, 11), (11, 23))


@pytest.mark.parametrize("spec,names", [([-1], "-1"), ([12], "12"), ([3, 40], "40"), ([], "empty"), ((), "empty"), ("first", "'first'"),
                                        (["mid", "5"], "'mid'"), (["5", "x"], "'x'"), ([1.5], "1.5"), ("", "''")])
def test_refusals_name_the_offender(spec, names):
    with pytest.raises(ValueError, match=names):
        resolve(spec, 12, 12)


def test_depths_that_cannot_be_paired():
    for spec in (None, "all", [0]):
        with pytest.raises(ValueError, match=r"18.*12"):
            resolve(spec, 12, 18)
    with pytest.raises(ValueError, match=r"6.*12"):
        resolve(None, 12, 6)


def test_cli_flag():
    import distill_sub
    p = argparse.ArgumentParser(parents=[distill_sub.get_args_parser()])
    assert p.parse_args([]).relation_layers == ["mid"]
    assert p.parse_args(["--relation-layers", "all"]).relation_layers == ["all"]
    assert p.parse_args(["--relation-layers", "0", "5", "11"]).relation_layers == ["0", "5", "11"]
    with pytest.raises(SystemExit):
        p.parse_args(["--relation-layers"])                                # nargs='+'

    class M:
        def __init__(self, n):
            self.blocks = [None] * n
    for argv, sl, tl, want in ((["mid"], 12, 24, (5,)), (["last"], 12, 12, (11,)), (["all"], 6, 12, tuple(range(6))), (["11", "0", "5", "5"], 12, 12, (0, 5, 11))):
        args = p.parse_args(["--relation-layers"] + argv)
        pairs = distill_sub.check_relation_layers(args, M(sl), M(tl))
        assert args.relation_layers == want and tuple(s for s, _ in pairs) == want
        assert pairs == resolve(want, sl, tl)
    for argv, sl, tl, names in ((["12"], 12, 12, "12"), (["-1"], 12, 12, "-1"), (["middle"], 12, 12, "'middle'"), (["mid", "last"], 12, 12, "'mid'"),
                                (["all"], 12, 18, r"18.*12")):
        args = p.parse_args(["--relation-layers"] + argv)
        with pytest.raises(SystemExit, match=names) as e:
            distill_sub.check_relation_layers(args, M(sl), M(tl))
        with pytest.raises(ValueError) as v:
            resolve(argv, sl, tl)
        assert str(v.value) in str(e.value) and "--relation-layers" in str(e.value)
    import ensemble                                                       # the flag belongs to the DEKD stage alone
    import train_subdata
    for other in (ensemble, train_subdata):
        q = argparse.ArgumentParser(parents=[other.get_args_parser()])
        assert not hasattr(q.parse_args([]), "relation_layers") and "--relation-layers" not in q.format_help()
        with pytest.raises(SystemExit):
            q.parse_args(["--relation-layers", "all"])
        assert q.parse_args(["--hid-gama", "0.5"]).hid_gama == 0.5        # (the flags they share stay)


def test_engine_refuses_a_bad_selection_before_any_forward():
    from devit_amd import engine

    class M(torch.nn.Module):
        def __init__(self, n):
            super().__init__()
            self.blocks = torch.nn.ModuleList(torch.nn.Identity() for _ in range(n))
    with pytest.raises(ValueError, match="12"):
        engine.distill_forward(M(12), M(12), None, None, relation_layers=[12])
    with pytest.raises(ValueError, match=r"18.*12"):
        engine.distill_forward(M(12), M(18), None, None)
    with pytest.raises(ValueError, match="'first'"):
        engine.TeacherLookahead(M(12), relation_layers="first", student_depth=12)
    look = engine.TeacherLookahead(M(24), relation_layers=[0, 5, 11], student_depth=12)
    assert look.layers == (1, 11, 23) and look.teacher.qkv_pad_layers == {1, 11, 23}
    assert engine.TeacherLookahead(M(24), student_depth=12).layers == (11,) and engine.TeacherLookahead(M(12)).layers == (5,)


@pytest.fixture(scope="module")
def step32():
    S, B, C = 32, 2, 25
    st_s, st_t = IM.make_state(GS, C, "S", S), IM.make_state(GT, C, "T", S)
    img = torch.from_numpy(det_array("rellayers/host32", (B, 3, S, S)))
    y = det_labels("rellayers/hy", B, C)
    soft = torch.full((B, C), 0.1 / C).scatter_(1, torch.from_numpy(y)[:, None], 1 - 0.1 + 0.1 / C)
    dps = IM.dp_scales_for("rellayers/host32", B)

    def run(fn, **kw):
        st = {k: v.clone().requires_grad_(True) for k, v in st_s.items()}
        out = fn(st, GS, st_t, GT, img, soft, dp_scales=dps, **kw)
        out["loss"].backward()
        return out, {k: v.grad for k, v in st.items()}
    return run


def test_helper_at_mid_is_the_imgsize_step_bit_for_bit(step32):
    ref, g_ref = step32(IM.distill_step)
    for layers in ("mid", [5]):
        out, g = step32(RM.distill_step, layers=layers)
        assert out["pairs"] == ((5, 5),)
        for k in ("loss", "cls_loss", "q_loss", "k_loss", "v_loss"):
            assert torch.equal(out[k], ref[k]), k
        assert [n for n in g_ref if g[n] is None or not torch.equal(g[n], g_ref[n])] == []
        assert torch.equal(out["rel_layers"][0] / 12, torch.stack([ref["q_loss"], ref["k_loss"], ref["v_loss"]]).detach())


def test_helper_sums_the_pairs(step32):
    """`all` is the sum of the single-layer steps' relation terms, and blocks above the selection get no relation gradient"""
    out, g = step32(RM.distill_step, layers="all")
    assert out["pairs"] == tuple((s, s) for s in range(12)) and tuple(out["rel_layers"].shape) == (12, 3)
    singles = [step32(RM.distill_step, layers=[s])[0] for s in (0, 5, 11)]
    for o, s in zip(singles, (0, 5, 11)):
        assert torch.equal(o["rel_layers"][0], out["rel_layers"][s])
    assert bool((out["rel_layers"] > 0).all())
    want = out["rel_layers"].double().sum(0) / 12
    for j, k in enumerate(("q_loss", "k_loss", "v_loss")):
        assert abs(float(out[k].detach()) - float(want[j])) <= 1e-6 * float(want[j])
    first, g0 = step32(RM.distill_step, layers=[0])
    cls_only, gc = step32(RM.distill_step, layers=[0], gama=(0., 0., 0.))
    assert torch.equal(g0["blocks.3.attn.qkv.weight"], gc["blocks.3.attn.qkv.weight"])
    assert not torch.equal(g0["blocks.0.attn.qkv.weight"], gc["blocks.0.attn.qkv.weight"])
