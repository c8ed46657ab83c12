"""Host side of the device-resident datasets (devit_amd/data.py, include/devit_hip.h "Input augmentation"): the numpy restatement of the
kernels (tests/_augment_model.py) against PIL -- the committed golden, and PIL live where it imports --, its derived bounds against an fp32
emulation and against planted bugs, the draws of TrainAugment against an independent scalar restatement of timm 0.5.4's formulas, the set
readers on trees written into tmp_path, and the refusals.  Nothing here needs a GPU."""
import argparse
import ctypes as C
import math
import os
import pickle
import random
import re

import numpy as np
import pytest

import _augment_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "augment_pil.npz")))


# ============================================================================================ the resampling against PIL
def test_model_equals_the_golden(gold):
    cases = M.golden_cases(gold)
    assert len(cases) >= 40
    sizes, filters = set(), set()
    for i, (img, r, S, px) in enumerate(cases):
        assert np.array_equal(M.resample(img, r, S), px), (i, r)
        sizes.add(S)
        filters.add(r["filter"])
    assert sizes == {32, 48, 224} and filters == {0, 1, 2}
    # the golden holds the cases the kernels are held to: a down-scaling pair, the eval geometries, the four padded corners, the degenerate boxes
    rows = [(r["y0"], r["x0"], r["h"], r["w"], r["Rh"], S, r["filter"]) for _, r, S, _ in cases]
    assert any(h == 48 and S == 32 and f == 1 for _, _, h, _, _, S, f in rows) and any(h == 48 and S == 32 and f == 2 for _, _, h, _, _, S, f in rows)
    assert any(Rh == 54 and S == 48 for *_, Rh, S, _ in rows) and any(Rh == 256 and S == 224 for *_, Rh, S, _ in rows)
    assert {(y, x) for y, x, *_, f in rows if f == 0} >= {(-4, -4), (-4, 4), (4, -4), (4, 4)}
    assert {(1, 5), (3, 3), (32, 32)} <= {(h, w) for _, _, h, w, *_ in rows}


def test_model_equals_pil_live(gold):
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.RandomState(11)
    n = 0
    for name, S_all in (("src32", (16, 32, 48)), ("src2028", (16, 48)), ("src48", (32,))):
        src = gold[name]
        H0, W0 = src.shape[1:3]
        for _ in range(100):
            S = int(rng.choice(S_all))
            h, w = int(rng.randint(1, H0 + 1)), int(rng.randint(1, W0 + 1))
            y0, x0, filt = int(rng.randint(0, H0 - h + 1)), int(rng.randint(0, W0 - w + 1)), int(rng.randint(1, 3))
            if max(M.taps_needed(h, S, filt), M.taps_needed(w, S, filt)) > M.TAPS:
                continue
            img = src[rng.randint(src.shape[0])]
            want = Image.fromarray(img).crop((x0, y0, x0 + w, y0 + h)).resize((S, S), {1: Image.BILINEAR, 2: Image.BICUBIC}[filt])
            assert np.array_equal(M.resample(img, M.row(y0, x0, h, w, S, filter=filt), S), np.asarray(want)), (name, y0, x0, h, w, S, filt)
            n += 1
    assert n >= 250


def test_product_tap_count_is_the_model_s():
    from devit_amd import data
    for length, R, filt in ((32, 224, 2), (32, 48, 1), (48, 32, 2), (80, 32, 2), (81, 32, 2), (160, 32, 1), (170, 32, 1), (5, 48, 2), (1, 32, 2)):
        assert data.taps_needed(length, R, filt) == M.taps_needed(length, R, filt), (length, R, filt)
    assert M.taps_needed(80, 32, 2) <= M.taps_needed(96, 32, 2) <= M.TAPS < M.taps_needed(112, 32, 2)       # 2.5 x and 3 x are served, 3.5 x is not


# ============================================================================================ bounds: hold for fp32, fail for planted bugs
def _erase_rows(S):
    return [M.row(3, 2, 20, 25, S, filter=2, flip=1, erase=[(5, 7, 9, 13)], erase_mode=M.CONST, noise_base=7),
            M.row(0, 0, 32, 32, S, filter=1, flip=0, erase=[(0, 0, 11, 6), (8, 3, 20, 30)], erase_mode=M.RAND, noise_base=1 << 40),
            M.row(9, 1, 7, 30, S, filter=2, flip=1, erase=[(30, 30, 18, 18), (1, 40, 10, 7), (33, 35, 5, 9), (0, 0, 3, 3)], erase_mode=M.PIXEL, noise_base=12345)]


def test_bounds_hold_for_an_fp32_emulation(gold):
    S, src = 48, gold["src32"]
    rows, idx = _erase_rows(S), [2, 0, 3]
    ref, bound = M.batch(src, idx, rows, S, MEAN, STD, seed=0x1234567890ABCDEF)
    emu, _ = M.batch(src, idx, rows, S, MEAN, STD, seed=0x1234567890ABCDEF, fp32=True)
    assert emu.shape == ref.shape == (3, 3, S, S)
    assert (np.abs(emu - ref) <= bound).all(), float((np.abs(emu - ref) / np.maximum(bound, 1e-300)).max())
    assert (emu != ref).any()                                   # the emulation does round
    assert bound[0].max() < 3e-6 and 5.9 * M.NOISE_ULPS * M.ULP < 7e-6     # the size of the bounds the docstring quotes
    # the noise is standard normal: mean and variance of the pixel-mode box of sample 2 (18 x 18 x 3 values)
    z = ref[2][:, 30:48, 30:48]
    assert abs(z.mean()) < 4 / math.sqrt(z.size) and abs(z.var() - 1) < 0.25


@pytest.mark.parametrize("bug", ["taps_escape", "vertical_first", "no_intermediate", "flip_before_crop", "erase_before_normalize", "wrong_channel"])
def test_bounds_catch_planted_bugs(gold, bug):
    S, src = 48, gold["src32"]
    rows, idx = _erase_rows(S), [2, 0, 3]
    ref, bound = M.batch(src, idx, rows, S, MEAN, STD, seed=99)
    bad, _ = M.batch(src, idx, rows, S, MEAN, STD, seed=99, bug=bug)
    assert (np.abs(bad - ref) > bound).any(), bug


# ============================================================================================ the draws
def _timm_draws(rng, B, H0, W0, S, scale, ratio, interpolation, hflip, re_prob, re_count):
    """timm 0.5.4, written out once more: RandomResizedCropAndInterpolation.get_params + __call__'s random.choice, RandomHorizontalFlip on the
    same generator, RandomErasing._erase -> [(i, j, h, w, filter, flip, boxes)]"""
    out = []
    for _ in range(B):
        if S == 32:
            i, j = rng.randint(0, H0 + 8 - S) - 4, rng.randint(0, W0 + 8 - S) - 4
            h, w, filt = S, S, 0
        else:
            area, got = W0 * H0, None
            for _ in range(10):
                target_area = rng.uniform(*scale) * area
                log_ratio = (math.log(ratio[0]), math.log(ratio[1]))
                aspect_ratio = math.exp(rng.uniform(*log_ratio))
                w = int(round(math.sqrt(target_area * aspect_ratio)))
                h = int(round(math.sqrt(target_area / aspect_ratio)))
                if w <= W0 and h <= H0:
                    i = rng.randint(0, H0 - h)
                    j = rng.randint(0, W0 - w)
                    got = (i, j, h, w)
                    break
            if got is None:
                in_ratio = W0 / H0
                if in_ratio < min(ratio):
                    w = W0
                    h = int(round(w / min(ratio)))
                elif in_ratio > max(ratio):
                    h = H0
                    w = int(round(h * max(ratio)))
                else:
                    w, h = W0, H0
                got = ((H0 - h) // 2, (W0 - w) // 2, h, w)
            i, j, h, w = got
            filt = rng.choice((1, 2)) if interpolation == 'random' else {'bilinear': 1, 'bicubic': 2}[interpolation]
        flip = int(rng.random() < hflip)
        boxes = []
        if re_prob > 0 and not rng.random() > re_prob:
            count = 1 if re_count == 1 else rng.randint(1, re_count)
            for _ in range(count):
                for _ in range(10):
                    target_area = rng.uniform(0.02, 1 / 3) * S * S / count
                    aspect_ratio = math.exp(rng.uniform(math.log(0.3), math.log(1 / 0.3)))
                    eh = int(round(math.sqrt(target_area * aspect_ratio)))
                    ew = int(round(math.sqrt(target_area / aspect_ratio)))
                    if ew < S and eh < S:
                        top = rng.randint(0, S - eh)
                        left = rng.randint(0, S - ew)
                        boxes.append((top, left, eh, ew))
                        break
        out.append((i, j, h, w, filt, flip, boxes))
    return out


@pytest.mark.parametrize("S,interp,re_prob,re_count,size", [(48, 'bicubic', 0.25, 1, (32, 32)), (224, 'random', 1.0, 4, (32, 32)),
                                                            (64, 'bilinear', 0.0, 1, (20, 28)), (32, 'bicubic', 0.5, 3, (32, 32))])
def test_train_draws_equal_the_timm_formulas(S, interp, re_prob, re_count, size):
    from devit_amd import data
    seed, rank, B = 5, 2, 37
    tf = data.TrainAugment(S, interpolation=interp, re_prob=re_prob, re_mode='pixel', re_count=re_count, seed=seed, rank=rank)
    rng = random.Random(seed * 65536 + rank)
    H0, W0 = size
    drawn = 0
    for _ in range(3):                                     # the stream carries on from batch to batch
        tab = tf.draw(B, H0, W0)
        want = _timm_draws(rng, B, H0, W0, S, (0.08, 1.0), (3 / 4, 4 / 3), interp, 0.5, re_prob, re_count)
        for b, (i, j, h, w, filt, flip, boxes) in enumerate(want):
            r = tab[b]
            assert (r["y0"], r["x0"], r["h"], r["w"], r["filter"], r["flip"], r["n_erase"]) == (i, j, h, w, filt, flip, len(boxes)), b
            assert [tuple(int(v) for v in e) for e in r["erase"][:len(boxes)]] == boxes and not r["erase"][len(boxes):].any()
            assert (r["Rh"], r["Rw"], r["oy"], r["ox"], r["erase_mode"]) == (S, S, 0, 0, 2)
        assert (tab["noise_base"] == (rank << 48) + drawn).all()
        drawn += B
        data.check_table(tab, H0, W0, S)                   # what is drawn is what the stage accepts
        # invariants: the box inside the image (the padded crop inside its padding), erase boxes strictly smaller than the output
        if S > 32:
            assert (tab["y0"] >= 0).all() and (tab["x0"] >= 0).all() and (tab["y0"] + tab["h"] <= H0).all() and (tab["x0"] + tab["w"] <= W0).all()
        else:
            assert (np.abs(tab["y0"]) <= 4).all() and (np.abs(tab["x0"]) <= 4).all()
        for r in tab:
            for top, left, eh, ew in r["erase"][:r["n_erase"]]:
                assert 1 <= eh < S and 1 <= ew < S and 0 <= top <= S - eh and 0 <= left <= S - ew
        if re_prob == 0.0:
            assert not tab["n_erase"].any()
        if re_prob == 1.0:
            assert (tab["n_erase"] >= 1).all() and tab["n_erase"].max() > 1


def test_crop_fallback_rule():
    from devit_amd import data
    # a scale no attempt can satisfy: ten failures, then the central crop with the ratio clamped
    tab = data.TrainAugment(48, scale=(4.0, 4.0), seed=1).draw(4, 32, 32)
    assert {(int(r["y0"]), int(r["x0"]), int(r["h"]), int(r["w"])) for r in tab} == {(0, 0, 32, 32)}
    tab = data.TrainAugment(48, scale=(4.0, 4.0), seed=1).draw(2, 20, 60)             # in_ratio 3 > 4/3: h = H0, w = round(h * 4/3) = 27
    assert {(int(r["y0"]), int(r["x0"]), int(r["h"]), int(r["w"])) for r in tab} == {(0, 16, 20, 27)}
    tab = data.TrainAugment(48, scale=(4.0, 4.0), seed=1).draw(2, 60, 20)             # in_ratio 1/3 < 3/4: w = W0, h = round(w / (3/4)) = 27
    assert {(int(r["y0"]), int(r["x0"]), int(r["h"]), int(r["w"])) for r in tab} == {(16, 0, 27, 20)}


def test_state_dict_round_trip():
    from devit_amd import data
    a = data.TrainAugment(48, re_prob=0.5, re_mode='rand', re_count=2, seed=3, rank=1)
    a.draw(10, 32, 32)
    state = pickle.loads(pickle.dumps(a.state_dict()))        # as a checkpoint stores it
    want = a.draw(16, 32, 32)
    b = data.TrainAugment(48, re_prob=0.5, re_mode='rand', re_count=2, seed=3, rank=1)
    b.load_state_dict(state)
    got = b.draw(16, 32, 32)
    assert got.tobytes() == want.tobytes() and int(got["noise_base"][0]) == (1 << 48) + 10
    c = data.TrainAugment(48, re_prob=0.5, re_mode='rand', re_count=2, seed=3, rank=0)
    assert c.draw(10, 32, 32).tobytes() != data.TrainAugment(48, re_prob=0.5, re_mode='rand', re_count=2, seed=3, rank=1).draw(10, 32, 32).tobytes()


def test_eval_geometry():
    from devit_amd import data
    assert data.EvalTransform(48).geometry(32, 32) == (54, 54, 3, 3, 2)
    assert data.EvalTransform(48).geometry(20, 28) == (54, 75, 3, 14, 2)
    assert data.EvalTransform(48).geometry(28, 20) == (75, 54, 14, 3, 2)
    assert data.EvalTransform(224).geometry(32, 32) == (256, 256, 16, 16, 2)
    assert data.EvalTransform(32).geometry(32, 32) == (32, 32, 0, 0, 0)
    tab = data.EvalTransform(48).draw(3, 20, 28)
    assert tab["h"].tolist() == [20] * 3 and tab["w"].tolist() == [28] * 3 and not tab["flip"].any() and not tab["n_erase"].any()
    data.check_table(tab, 20, 28, 48)


# ============================================================================================ the set readers
def test_from_cifar100(tmp_path):
    from devit_amd import data
    d = tmp_path / "cifar-100-python"
    d.mkdir()
    rng = np.random.RandomState(0)
    for name, n in (("train", 7), ("test", 3)):
        raw = rng.randint(0, 256, (n, 3072)).astype(np.uint8)
        with open(d / name, "wb") as f:
            pickle.dump({"data": raw, "fine_labels": list(range(n)), "coarse_labels": [0] * n}, f)
        if name == "train":
            train_raw = raw
    with open(d / "meta", "wb") as f:
        pickle.dump({"fine_label_names": [f"c{i}" for i in range(100)]}, f)
    s = data.DeviceImageSet.from_cifar100(str(tmp_path), True, device="cpu")
    assert len(s) == 7 and s.size == (32, 32) and s.images.dtype.is_floating_point is False and s.labels.tolist() == list(range(7))
    assert s.classes[:2] == ["c0", "c1"] and len(s.classes) == 100
    assert np.array_equal(s.images[4, 5, 6].numpy(), train_raw[4].reshape(3, 32, 32)[:, 5, 6])       # CHW in the pickle, HWC resident
    assert len(data.DeviceImageSet.from_cifar100(str(tmp_path), False, device="cpu")) == 3
    with pytest.raises(SystemExit, match="cifar-100-python"):
        data.DeviceImageSet.from_cifar100(str(tmp_path / "nowhere"), True, device="cpu")


def test_from_folder(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    from devit_amd import data
    rng = np.random.RandomState(1)
    want = {}
    for c in ("zebra", "ant", "bee"):
        (tmp_path / "set" / c).mkdir(parents=True)
        for fn in ("2.png", "10.png", "1.png"):
            a = rng.randint(0, 256, (20, 28, 3)).astype(np.uint8)
            Image.fromarray(a).save(tmp_path / "set" / c / fn)
            want[(c, fn)] = a
    (tmp_path / "set" / "ant" / "notes.txt").write_text("not an image")
    Image.fromarray(want[("bee", "1.png")][:, :, 0]).save(tmp_path / "set" / "bee" / "0_grey.png")       # mode L: convert('RGB')
    s = data.DeviceImageSet.from_folder(str(tmp_path / "set"), device="cpu")
    assert s.classes == ["ant", "bee", "zebra"] and s.size == (20, 28) and len(s) == 10
    assert s.labels.tolist() == [0] * 3 + [1] * 4 + [2] * 3
    order = [("ant", "1.png"), ("ant", "10.png"), ("ant", "2.png")]                      # sorted as strings, like ImageFolder
    for i, key in enumerate(order):
        assert np.array_equal(s.images[i].numpy(), want[key])
    grey = s.images[3].numpy()
    assert np.array_equal(grey[:, :, 0], want[("bee", "1.png")][:, :, 0]) and np.array_equal(grey[:, :, 0], grey[:, :, 2])
    Image.fromarray(np.zeros((21, 28, 3), np.uint8)).save(tmp_path / "set" / "zebra" / "9.png")
    with pytest.raises(ValueError, match="resident sets are uniform"):
        data.DeviceImageSet.from_folder(str(tmp_path / "set"), device="cpu")


# ============================================================================================ refusals
def test_refusals():
    from devit_amd import data
    with pytest.raises(ValueError, match="resident sets are uniform"):
        data.DeviceImageSet.from_arrays([np.zeros((32, 32, 3), np.uint8), np.zeros((32, 31, 3), np.uint8)], [0, 1], device="cpu")
    with pytest.raises(ValueError, match="uint8"):
        data.DeviceImageSet.from_arrays(np.zeros((2, 32, 32, 3), np.float32), [0, 1], device="cpu")
    with pytest.raises(ValueError, match="re_count 5"):
        data.TrainAugment(48, re_prob=0.5, re_count=5)
    with pytest.raises(ValueError, match="re_mode"):
        data.TrainAugment(48, re_mode='noise')
    with pytest.raises(ValueError, match="interpolation"):
        data.TrainAugment(48, interpolation='lanczos')
    with pytest.raises(ValueError):
        data.TrainAugment(40)                                            # not one of ops.IMG_SIZES
    s = data.DeviceImageSet.from_arrays(np.zeros((4, 160, 160, 3), np.uint8), [0, 1, 2, 3], device="cpu")
    with pytest.raises(ValueError, match="needs 14 taps .* holds 12"):
        data.DeviceLoader(s, range(4), 2, data.TrainAugment(48), drop_last=True)
    data.DeviceLoader(s, range(4), 2, data.EvalTransform(48), drop_last=False)           # 160 -> 54: 12 taps
    with pytest.raises(ValueError, match="EvalTransform on 240 x 240 .* taps"):
        data.EvalTransform(48).check_set(240, 240)
    data.DeviceLoader(s, range(4), 2, data.TrainAugment(64), drop_last=True)             # 2.5 x (11 taps): served
    with pytest.raises(ValueError, match="as they are"):
        data.DeviceLoader(s, range(4), 2, data.EvalTransform(32), drop_last=False)
    ld = data.DeviceLoader(s, range(4), 3, data.TrainAugment(64), drop_last=True)
    assert len(ld) == 1 and len(data.DeviceLoader(s, range(4), 3, data.TrainAugment(64), drop_last=False)) == 2 and ld.sampler == range(4)
    good = data.TrainAugment(48, seed=1).draw(4, 32, 32)
    for field, value, msg in (("filter", 3, "filter"), ("n_erase", 5, "n_erase"), ("h", 0, "empty"), ("oy", 1, "window"), ("y0", 30, "inside the 32 x 32"),
                              ("x0", -1, "inside the 32 x 32")):
        bad = good.copy()
        bad[field][1] = value
        with pytest.raises(ValueError, match=msg):
            data.check_table(bad, 32, 32, 48)


def _args(argv):
    import distill_sub
    return argparse.ArgumentParser(parents=[distill_sub.get_args_parser()]).parse_args(argv)


def test_cli_refusals(tmp_path):
    import distill_sub
    ok = ["--device-data", "--aa", "none", "--color-jitter", "0", "--input-size", "48"]
    distill_sub.check_device_data(_args(ok))
    distill_sub.check_device_data(_args(["--aa", "rand-m9-mstd0.5-inc1"]))               # without the flag nothing is checked
    for extra, msg in ((["--aa", "rand-m9-mstd0.5-inc1"], "RandAugment"), (["--color-jitter", "0.4"], "ColorJitter"), (["--no_aug"], "--no_aug"),
                       (["--synthetic", "2"], "--synthetic"), (["--recount", "5"], "--recount 5"), (["--remode", "noise"], "--remode"),
                       (["--train-interpolation", "lanczos"], "--train-interpolation")):
        with pytest.raises(SystemExit, match=msg):
            distill_sub.check_device_data(_args(ok + extra))
    with pytest.raises(SystemExit, match="RandAugment.*ColorJitter"):                     # the defaults ask for both: both are named
        distill_sub.check_device_data(_args(["--device-data"]))
    distill_sub.check_device_data(_args(["--device-data", "--aa", "", "--color-jitter", "0"]))
    with pytest.raises(SystemExit, match="--dataset cars"):
        distill_sub.build_loaders(_args(ok + ["--dataset", "cars"]), 196, "cpu", provider="whole", plain_sampler_over="train")
    with pytest.raises(SystemExit, match="not a directory"):
        distill_sub.build_loaders(_args(ok + ["--data-path", str(tmp_path)]), 25, "cpu", provider="division")
    with pytest.raises(SystemExit, match="cifar-100-python"):
        distill_sub.build_loaders(_args(ok + ["--data-path", str(tmp_path)]), 100, "cpu", provider="whole", plain_sampler_over="train")
    for script in ("train_subdata.py", "ensemble.py"):                                    # the flag reaches the other two CLIs
        assert "ds.get_args_parser()" in open(os.path.join(ROOT, script)).read()


def test_division_loaders_on_a_folder_tree(tmp_path):
    """build_loaders(--device-data) over <data-path>/sub-dataset<k>/{train_dataset,test_dataset}: samplers, drop_last and the --no-repeated-aug quirk as
    the host loaders have them (on the CPU: nothing is iterated)."""
    Image = pytest.importorskip("PIL.Image")
    import distill_sub
    import torch
    for split, per_class in (("train_dataset", 300), ("test_dataset", 3)):
        for c in ("a", "b"):
            (tmp_path / "sub-dataset1" / split / c).mkdir(parents=True)
            for i in range(per_class if c == "a" else 2):
                Image.fromarray(np.full((32, 32, 3), i % 256, np.uint8)).save(tmp_path / "sub-dataset1" / split / c / f"{i}.png")
    base = ["--device-data", "--aa", "none", "--color-jitter", "0", "--input-size", "48", "--data-path", str(tmp_path), "--start-division", "1", "--batch-size", "4",
            "--eval-batch-size", "4", "--reprob", "0.25", "--seed", "9"]
    tr, va, nc = distill_sub.build_loaders(_args(base), 25, "cpu", provider="division")
    assert nc == 2 and isinstance(tr.sampler, distill_sub.RASampler) and len(tr.sampler) == 256 and len(tr) == 64 and tr.drop_last
    assert isinstance(va.sampler, torch.utils.data.SequentialSampler) and len(va) == 2 and not va.drop_last
    assert tr.transform.S == 48 and tr.transform.re_prob == 0.25 and tr.transform.re_mode == 'pixel' and tr.transform.seed == 9
    tr2, _, _ = distill_sub.build_loaders(_args(base + ["--no-repeated-aug"]), 25, "cpu", provider="division")
    assert isinstance(tr2.sampler, torch.utils.data.DistributedSampler) and len(tr2.sampler) == 5          # over the TEST set: the quirk, kept
    assert distill_sub.loader_state(tr)["drawn"] == 0 and distill_sub.loader_state(object()) == {}


# ============================================================================================ ABI
def test_table_row_layout():
    """header struct, ctypes mirror and numpy mirror of devit_augment_sample agree field by field (test_abi.py holds symbols, count and sizeof)."""
    from devit_amd import _lib, data
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "devit_hip.h")).read(), flags=re.S)
    end = src.index("} devit_augment_sample;")
    body = src[src.rindex("typedef struct {", 0, end) + len("typedef struct {"):end]
    names = []
    for stmt in body.split(";"):
        for piece in stmt.split(","):
            ids = re.findall(r"[A-Za-z_][A-Za-z0-9_]*", re.sub(r"\[.*", "", piece))
            if ids:
                names.append(ids[-1])
    assert names == [f[0] for f in _lib.AugmentSample._fields_] == list(data.AUG_SAMPLE_DTYPE.names)
    assert C.sizeof(_lib.AugmentSample) == data.AUG_SAMPLE_DTYPE.itemsize == 120
    for n in names:
        assert getattr(_lib.AugmentSample, n).offset == data.AUG_SAMPLE_DTYPE.fields[n][1], n
    assert _lib.ABI_STRUCTS[14] is _lib.AugmentSample and "devit_augment_batch" in _lib.SIGNATURES
    assert (_lib.AUGMENT_TAPS, _lib.AUGMENT_MAX_ERASE, _lib.AUGMENT_SITE) == (M.TAPS, M.MAX_ERASE, M.SITE)
    for macro, value in (("DEVIT_AUGMENT_TAPS", 12), ("DEVIT_AUGMENT_MAX_ERASE", 4), ("DEVIT_AUGMENT_SITE", 0x100)):
        assert int(re.search(r"#define %s (\w+)" % macro, src).group(1).rstrip("u"), 0) == value
