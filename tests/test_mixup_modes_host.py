"""Host side of the per-sample Mixup / CutMix modes (timm Mixup mode='elem' / 'pair', cutmix_minmax): argument checks, the
properties and the RNG call order of Mixup.draw_table, ops.mix_table's validation, and the flags reaching Mixup from each CLI.
No GPU: nothing here launches a kernel."""
import argparse
import ctypes as C
import math

import numpy as np
import pytest

import distill_sub
import ensemble
import train_subdata
from devit_amd import _lib, ops
from distill_sub import Mixup

H = W = 224
FIELDS = ("mode", "lam", "y0", "y1", "x0", "x1")


def mk(ma=0.8, ca=1.0, prob=1.0, sw=0.5, **kw):
    return Mixup(ma, ca, prob, sw, 0.1, 10, **kw)


# ------------------------------------------------------------------------------------------ construction
def test_constructor_refuses_bad_settings():
    with pytest.raises(ValueError):
        mk(mode="nope")
    for bad in ((0.5,), (0.8, 0.2), (0.5, 0.5), (-0.1, 0.5), (0.2, 1.5), (0.1, 0.2, 0.3)):
        with pytest.raises(ValueError):
            mk(cutmix_minmax=bad)
    for mode in ("batch", "elem", "pair"):
        assert mk(mode=mode).mode == mode
    m = mk()                                      # today's positional call: batch mode, area-ratio box
    assert m.mode == "batch" and m.cutmix_minmax is None and m.ca == 1.0


def test_minmax_forces_cutmix_alpha_one():
    m = mk(ca=0.3, cutmix_minmax=(0.2, 0.8))
    assert m.ca == 1.0 and m.cutmix_minmax == (0.2, 0.8)
    assert mk(ca=0.0, cutmix_minmax=[0.2, 0.8], mode="elem").ca == 1.0


def test_abi_mirror_of_the_table_entry():
    assert C.sizeof(_lib.MixSample) == 32 == ops.MIX_SAMPLE_DTYPE.itemsize and _lib.ABI_STRUCTS[10] is _lib.MixSample
    assert [f[0] for f in _lib.MixSample._fields_] == list(ops.MIX_SAMPLE_DTYPE.names)
    assert [getattr(_lib.MixSample, n).offset for n in FIELDS] == [ops.MIX_SAMPLE_DTYPE.fields[n][1] for n in FIELDS]
    assert {"devit_mix_im2row_table", "devit_mix_targets_table"} <= set(_lib.SIGNATURES)


# ------------------------------------------------------------------------------------------ draw_table: properties of every draw
B = 8
SEEDS = range(40)           # each property holds for every draw: more seeds only visit more branches


def tables(**kw):
    m = mk(**kw)
    for s in SEEDS:
        np.random.seed(s)
        yield m.draw_table(B)


def test_draw_table_prob_zero_mixes_nothing():
    for mode in ("elem", "pair"):
        for t in tables(prob=0.0, mode=mode):
            assert t.dtype == ops.MIX_SAMPLE_DTYPE and t.shape == (B,)
            assert (t["mode"] == 0).all() and (t["lam"] == 1).all()


def test_draw_table_mixup_only_and_cutmix_only():
    for mode in ("elem", "pair"):
        for t in tables(ca=0.0, mode=mode):
            assert (t["mode"] != 2).all() and (t["mode"] == 1).any()
        for t in tables(ma=0.0, mode=mode):
            assert np.isin(t["mode"], (0, 2)).all() and (t["mode"] == 2).any()


def test_draw_table_modes_follow_lam():
    seen = set()
    for kw in (dict(), dict(prob=0.5), dict(cutmix_minmax=(0.2, 0.8))):
        for t in tables(mode="elem", **kw):
            assert ((t["mode"] == 0) == (t["lam"] == 1)).all()
            assert ((t["lam"] >= 0) & (t["lam"] <= 1)).all()
            seen |= set(t["mode"].tolist())
    assert seen == {0, 1, 2}


def test_draw_table_pair_is_mirrored():
    for kw in (dict(), dict(cutmix_minmax=(0.2, 0.8)), dict(prob=0.5)):
        for t in tables(mode="pair", **kw):
            for i in range(B):
                assert t[i] == t[B - 1 - i]


def test_draw_table_cutmix_lam_is_the_box_area():
    n = 0
    for kw in (dict(mode="elem"), dict(mode="pair"), dict(mode="elem", cutmix_minmax=(0.2, 0.8))):
        for t in tables(**kw):
            for e in t[t["mode"] == 2]:
                area = (int(e["y1"]) - int(e["y0"])) * (int(e["x1"]) - int(e["x0"]))
                assert e["lam"] == np.float32(1 - area / (224 * 224)) and e["lam"].dtype == np.float32
                assert 0 <= e["y0"] <= e["y1"] <= H and 0 <= e["x0"] <= e["x1"] <= W
                n += 1
    assert n > 100


@pytest.mark.parametrize("mm", [(0.2, 0.8), (0.0, 1.0), (0.5, 0.51)])
def test_draw_table_minmax_box_sides(mm):
    n = 0
    for mode in ("elem", "pair"):
        for t in tables(mode=mode, cutmix_minmax=mm):
            for e in t[t["mode"] == 2]:
                assert int(224 * mm[0]) <= e["y1"] - e["y0"] < int(224 * mm[1])
                assert int(224 * mm[0]) <= e["x1"] - e["x0"] < int(224 * mm[1])
                assert 0 <= e["y0"] and e["y1"] <= H and 0 <= e["x0"] and e["x1"] <= W
                n += 1
    assert n > 100


def test_batch_mode_minmax_changes_only_the_box_draw():
    """batch mode draws (rand < prob, rand < switch, beta) as before; with min/max the box is rand_bbox_minmax's and lam its area."""
    plain, mm = mk(), mk(cutmix_minmax=(0.2, 0.6))
    cuts = 0
    for s in SEEDS:
        np.random.seed(s)
        mode0, lam0, _ = plain.draw()
        np.random.seed(s)
        mode1, lam1, box = mm.draw()
        assert mode0 == mode1
        if mode1 == 2:
            np.random.seed(s)
            np.random.rand(), np.random.rand(), np.random.beta(1.0, 1.0)
            ch, cw = np.random.randint(int(H * 0.2), int(H * 0.6)), np.random.randint(int(W * 0.2), int(W * 0.6))
            yl, xl = np.random.randint(0, H - ch), np.random.randint(0, W - cw)
            assert box == (yl, yl + ch, xl, xl + cw) and lam1 == 1.0 - ch * cw / float(H * W)
            cuts += 1
        else:
            assert lam0 == lam1
    assert cuts > 5


# ------------------------------------------------------------------------------------------ draw_table: the order of the RNG calls
def restated_table(ma, ca, prob, sw, minmax, mode, Bn):
    """The order of draws of timm's Mixup._params_per_elem and of the box draws of _mix_elem / _mix_pair, written out: what
    draw_table must reproduce call for call on the numpy global RNG."""
    n = Bn // 2 if mode == "pair" else Bn
    lam = np.ones(n, dtype=np.float32)
    use_cutmix = np.zeros(n, dtype=bool)
    if ma > 0 and ca > 0:
        use_cutmix = np.random.rand(n) < sw
        beta_cut = np.random.beta(ca, ca, size=n)              # both vectors are drawn, cutmix first
        beta_mix = np.random.beta(ma, ma, size=n)
        lam_mix = np.where(use_cutmix, beta_cut, beta_mix)
    elif ma > 0:
        lam_mix = np.random.beta(ma, ma, size=n)
    else:
        use_cutmix = np.ones(n, dtype=bool)
        lam_mix = np.random.beta(ca, ca, size=n)
    lam = np.where(np.random.rand(n) < prob, lam_mix.astype(np.float32), lam)
    out = [None] * Bn
    for i in range(n):
        if lam[i] == 1:
            e = (0, np.float32(1), 0, 0, 0, 0)
        elif not use_cutmix[i]:
            e = (1, lam[i], 0, 0, 0, 0)
        else:
            if minmax is not None:
                cut_h = np.random.randint(int(H * minmax[0]), int(H * minmax[1]))
                cut_w = np.random.randint(int(W * minmax[0]), int(W * minmax[1]))
                yl = np.random.randint(0, H - cut_h)
                xl = np.random.randint(0, W - cut_w)
                y0, y1, x0, x1 = yl, yl + cut_h, xl, xl + cut_w
            else:
                ratio = np.sqrt(np.float32(1) - lam[i])
                cut_h, cut_w = int(np.float32(H) * ratio), int(np.float32(W) * ratio)
                cy = np.random.randint(H)
                cx = np.random.randint(W)
                y0, y1 = int(np.clip(cy - cut_h // 2, 0, H)), int(np.clip(cy + cut_h // 2, 0, H))
                x0, x1 = int(np.clip(cx - cut_w // 2, 0, W)), int(np.clip(cx + cut_w // 2, 0, W))
            e = (2, np.float32(1.0 - (y1 - y0) * (x1 - x0) / float(H * W)), y0, y1, x0, x1)
        out[i] = e
        if mode == "pair":
            out[Bn - 1 - i] = e
    return out


@pytest.mark.parametrize("mode", ["elem", "pair"])
@pytest.mark.parametrize("seed", [0, 7, 20240807])
@pytest.mark.parametrize("kw", [dict(), dict(cutmix_minmax=(0.2, 0.8)), dict(prob=0.6, sw=0.3), dict(ca=0.0), dict(ma=0.0)],
                         ids=["default", "minmax", "prob", "mixup_only", "cutmix_only"])
def test_draw_table_rng_order(mode, seed, kw):
    m = mk(mode=mode, **kw)
    np.random.seed(seed)
    got = m.draw_table(6)
    after = np.random.rand()                       # ... and not one draw more or less
    np.random.seed(seed)
    want = restated_table(m.ma, m.ca, m.prob, m.sw, m.cutmix_minmax, mode, 6)
    assert np.random.rand() == after
    for i, e in enumerate(want):
        for name, v in zip(FIELDS, e):
            assert got[i][name] == v and not math.isnan(got[i]["lam"]), (i, name, got[i], e)
    assert (got["reserved"] == 0).all()


def test_draw_table_needs_an_even_batch():
    with pytest.raises(AssertionError, match="Batch size should be even when using this"):
        mk(mode="pair").draw_table(5)


# ------------------------------------------------------------------------------------------ ops.mix_table validates before any device work
GOOD = [(0, 1.0, 0, 0, 0, 0), (1, 0.3, 0, 0, 0, 0), (2, 0.5, 10, 100, 3, 224), (2, 1.0, 5, 5, 0, 0)]


@pytest.mark.parametrize("bad", [(3, 0.5, 0, 0, 0, 0), (-1, 0.5, 0, 0, 0, 0), (1, -0.1, 0, 0, 0, 0), (1, 1.5, 0, 0, 0, 0),
                                 (1, float("nan"), 0, 0, 0, 0), (2, 0.5, 0, 225, 0, 10), (2, 0.5, 0, 10, 9, 8), (2, 0.5, -1, 10, 0, 8),
                                 (2, 0.5, 0, 10, 0, 225), (2, 0.5, 11, 10, 0, 8)])
def test_mix_table_refuses_bad_entries_on_the_host(monkeypatch, bad):
    reached = []
    monkeypatch.setattr(ops, "call", lambda *a: reached.append(a))
    for entries in (GOOD + [bad], [bad] + GOOD):
        with pytest.raises(ValueError):
            ops.mix_table(entries)
        arr = np.zeros(len(entries), dtype=ops.MIX_SAMPLE_DTYPE)
        for n, col in zip(FIELDS, zip(*entries)):
            arr[n] = col
        with pytest.raises(ValueError):
            ops.mix_table(arr)
    assert reached == []


def test_mix_entries_accepts_lists_and_structured_arrays():
    host = ops.mix_entries(GOOD)
    assert host.dtype == ops.MIX_SAMPLE_DTYPE and host.nbytes == 32 * len(GOOD)
    assert host["lam"].tolist() == [np.float32(v[1]) for v in GOOD] and host["x1"].tolist() == [0, 0, 224, 0]
    again = ops.mix_entries(host)
    assert again.tobytes() == host.tobytes()
    np.random.seed(3)
    t = mk(mode="elem").draw_table(8)
    assert ops.mix_entries(t).tobytes() == t.tobytes()
    with pytest.raises(ValueError):
        ops.mix_entries([])
    with pytest.raises(ValueError):
        ops.mix_entries([(1, 0.5)])


# ------------------------------------------------------------------------------------------ the flags reach Mixup from every CLI
def _parse(mod, argv):
    return argparse.ArgumentParser(parents=[mod.get_args_parser()], conflict_handler="resolve").parse_args(argv)


@pytest.mark.parametrize("mod", [distill_sub, train_subdata, ensemble], ids=lambda m: m.__name__)
def test_build_mixup_carries_the_flags(mod):
    m = distill_sub.build_mixup(_parse(mod, ["--mixup-mode", "pair", "--cutmix-minmax", "0.2", "0.6"]), 25)
    assert isinstance(m, Mixup) and m.mode == "pair" and m.cutmix_minmax == (0.2, 0.6) and m.ca == 1.0 and m.C == 25
    a = _parse(mod, [])
    m = distill_sub.build_mixup(a, 25)
    assert m.mode == "batch" and m.cutmix_minmax is None
    assert (m.ma, m.ca, m.prob, m.sw, m.eps) == (a.mixup, a.cutmix, a.mixup_prob, a.mixup_switch_prob, a.smoothing)
    assert distill_sub.build_mixup(_parse(mod, ["--mixup", "0", "--cutmix", "0"]), 25) is None
    assert distill_sub.build_mixup(_parse(mod, ["--mixup", "0", "--cutmix", "0", "--cutmix-minmax", "0.1", "0.5"]), 25).ca == 1.0
    with pytest.raises(ValueError):
        distill_sub.build_mixup(_parse(mod, ["--mixup-mode", "nope"]), 25)


def test_every_cli_builds_its_mixup_through_build_mixup():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for f in ("distill_sub.py", "train_subdata.py", "ensemble.py"):
        src = open(os.path.join(root, f)).read()
        assert "build_mixup(args, num_classes)" in src
        assert len(re.findall(r"\bMixup\(args\.", src)) == (1 if f == "distill_sub.py" else 0), f
