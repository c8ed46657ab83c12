"""CPU checks of the packed-set form of the input stage ("Packed sets" in include/devit_hip.h): tests/_ragged_model.py against PIL's results
(tests/golden/augment_ragged_pil.npz, and PIL live where it imports), its planted bugs, the closed-form tap bound, the draws on per-sample
sizes, the packed DeviceImageSet (arrays, folders, budget, save / load), the refusals, the CLI paths and the struct layout.  No GPU."""
import argparse
import ctypes as C
import math
import os
import random
import re

import numpy as np
import pytest
import torch

import _augment_model as M
import _ragged_model as RM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "augment_ragged_pil.npz")))


@pytest.fixture(scope="module")
def packed(gold):
    images, cases = RM.golden_set(gold)
    arena, entries = RM.pack(images)
    return images, cases, arena, entries


# ============================================================================================ the model against PIL
def test_model_equals_the_golden(packed):
    images, cases, arena, entries = packed
    assert sorted({im.shape[:2] for im in images}) == sorted([(20, 28), (33, 35), (200, 61), (61, 330), (150, 170), (40, 700), (146, 145)])
    taps = set()
    for i, r, S, px in cases:
        assert r["h"] <= 16 * r["w"]
        assert np.array_equal(RM.window(arena, entries, i, r, S), px), (i, r)
        taps.add(max(M.taps_needed(r["h"], r["Rh"], r["filter"]), M.taps_needed(r["w"], r["Rw"], r["filter"])))
    assert len(cases) >= 45 and {S for _, _, S, _ in cases} == {32, 48, 224}
    assert min(taps) == 1 and {12, 13, 14, 25, 28, 42} <= taps and max(taps) > 50          # exact counts (the closed-form bound may say one more)
    # the cases the file exists for
    whole = {(images[i].shape[:2], S, r["filter"]): r for i, r, S, _ in cases if (r["h"], r["w"]) == images[i].shape[:2] and r["Rh"] == S and r["Rw"] == S}
    r = whole[((146, 145), 48, M.BICUBIC)]
    assert (M.taps_needed(146, 48, M.BICUBIC), M.taps_needed(145, 48, M.BICUBIC)) == (13, 12) and RM.is_wide(r)
    assert (M.taps_needed(61, 48, M.BICUBIC), M.taps_needed(330, 48, M.BICUBIC)) == (6, 28)                 # narrow on one axis, wide on the other
    assert M.taps_needed(330, 32, M.BICUBIC) == 42 and M.taps_needed(200, 32, M.BICUBIC) == 25 and M.taps_needed(700, 224, M.BICUBIC) == 13
    assert (RM.taps_bound(330, 32, M.BICUBIC), RM.taps_bound(200, 32, M.BICUBIC), RM.taps_bound(700, 224, M.BICUBIC)) == (42, 26, 13)
    assert sum(RM.is_wide(r) for _, r, _, _ in cases) >= 10 and sum(not RM.is_wide(r) for _, r, _, _ in cases) >= 10


def test_model_equals_pil_live():
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.RandomState(5)
    for k in range(14):
        H, W = int(rng.randint(8, 260)), int(rng.randint(8, 260))
        img = rng.randint(0, 256, (H, W, 3)).astype(np.uint8)
        h = int(rng.randint(1, H + 1))
        w = int(rng.randint(max(1, (h + 15) // 16), W + 1))
        y0, x0, S, filt = int(rng.randint(0, H - h + 1)), int(rng.randint(0, W - w + 1)), (32, 48)[k % 2], (M.BILINEAR, M.BICUBIC)[k // 2 % 2]
        want = np.asarray(Image.fromarray(img).crop((x0, y0, x0 + w, y0 + h)).resize((S, S), {M.BILINEAR: Image.BILINEAR, M.BICUBIC: Image.BICUBIC}[filt]))
        assert np.array_equal(RM.resample(img, M.row(y0, x0, h, w, S, filter=filt), S), want), (H, W, y0, x0, h, w, S, filt)


@pytest.mark.parametrize("bug", RM.BUGS)
def test_planted_bugs_change_bytes(packed, bug):
    images, cases, arena, entries = packed
    changed = sum(not np.array_equal(RM.window(arena, entries, i, r, S, bug), px) for i, r, S, px in cases if S < 224)
    assert changed >= 3, (bug, changed)


def test_an_entry_outside_the_arena_reads_zeros(packed):
    images, cases, arena, entries = packed
    bad = list(entries)
    bad[3] = (arena.size - 100, 61, 330)
    i, r, S, _ = next(c for c in cases if c[0] == 3)
    assert not RM.window(arena, bad, 3, r, S).any() and RM.window(arena, entries, 3, r, S).any()
    assert np.array_equal(RM.fetch(arena, entries, 99), images[-1]) and np.array_equal(RM.fetch(arena, entries, -2), images[0])      # idx is clamped


# ============================================================================================ the tap bound
def test_tap_bound_brackets_the_exact_count():
    from devit_amd import _lib, data
    assert (_lib.AUGMENT_TAPS, _lib.AUGMENT_TAPS_MAX, _lib.AUGMENT_FORCE_WIDE) == (RM.TAPS, RM.TAPS_MAX, 1) and M.TAPS == 12
    lengths = list(range(1, 700)) + [1000, 1601, 2048, 4097, 7168, 7169]
    for R in (32, 48, 64, 73, 224, 256):
        for filt in (M.BILINEAR, M.BICUBIC):
            got = data.taps_bound(np.asarray(lengths), R, filt)
            for n, g in zip(lengths, got):
                exact = M.taps_needed(n, R, filt) if n < 700 or R >= 224 else None
                assert g == RM.taps_bound(n, R, filt)
                if exact is not None:
                    assert exact <= g <= exact + 1, (n, R, filt, exact, g)
    assert data.taps_bound(50, 50, M.NONE) == 1 and RM.taps_bound(50, 50, M.NONE) == 1
    assert data.taps_bound(7168, 224, M.BICUBIC) <= 129 and M.taps_needed(7168, 224, M.BICUBIC) == 128


# ============================================================================================ the draws
KW = dict(interpolation='random', re_prob=0.7, re_mode='pixel', re_count=3, seed=4, rank=1)


@pytest.mark.parametrize("S", [32, 48])
@pytest.mark.parametrize("aug", [{}, {"auto_augment": "rand-m9-mstd0.5-inc1"}, {"color_jitter": 0.4}])
def test_constant_size_arrays_draw_todays_tables(S, aug):
    from devit_amd import data
    a, b = data.TrainAugment(S, **KW, **aug), data.TrainAugment(S, **KW, **aug)
    for B in (5, 3):
        ta, la = a.draw_with_ops(B, 40, 52)
        tb, lb = b.draw_with_ops(B, np.full(B, 40), np.full(B, 52, dtype=np.int32))
        assert ta.tobytes() == tb.tobytes() and (la is None) == (lb is None) and (la is None or la.tobytes() == lb.tobytes())
    assert a.state_dict() == b.state_dict()
    e = data.EvalTransform(48)
    assert e.draw(4, 40, 52).tobytes() == e.draw(4, np.full(4, 40), np.full(4, 52)).tobytes()
    with pytest.raises(ValueError, match="3 image sizes for 4"):
        a.draw_with_ops(4, np.full(3, 40), np.full(3, 52))


def _crop_restated(rng, H0, W0, scale=(0.08, 1.0), ratio=(3. / 4., 4. / 3.)):
    """timm's RandomResizedCropAndInterpolation.get_params, restated"""
    for _ in range(10):
        target = rng.uniform(*scale) * (W0 * H0)
        ar = math.exp(rng.uniform(math.log(ratio[0]), math.log(ratio[1])))
        w, h = int(round(math.sqrt(target * ar))), int(round(math.sqrt(target / ar)))
        if w <= W0 and h <= H0:
            return rng.randint(0, H0 - h), rng.randint(0, W0 - w), h, w
    r = W0 / H0
    if r < ratio[0]:
        w, h = W0, int(round(W0 / ratio[0]))
    elif r > ratio[1]:
        h, w = H0, int(round(H0 * ratio[1]))
    else:
        w, h = W0, H0
    return (H0 - h) // 2, (W0 - w) // 2, h, w


def test_mixed_sizes_draw_each_sample_on_its_own_size():
    from devit_amd import data
    H, W = np.array([20, 200, 61, 700, 33, 1200]), np.array([28, 61, 330, 40, 35, 1600])
    tf = data.TrainAugment(48, interpolation='bicubic', hflip=0.5, seed=11, rank=2)
    tab = tf.draw(6, H, W)
    rng = random.Random(11 * 65536 + 2)
    for b in range(6):
        y0, x0, h, w = _crop_restated(rng, int(H[b]), int(W[b]))
        flip = int(rng.random() < 0.5)
        assert (tab["y0"][b], tab["x0"][b], tab["h"][b], tab["w"][b], tab["flip"][b]) == (y0, x0, h, w, flip), b
        assert 0 <= y0 and y0 + h <= H[b] and 0 <= x0 and x0 + w <= W[b]
    assert (tab["noise_base"] == (2 << 48)).all() and tf.drawn == 6
    pad = data.TrainAugment(32, seed=3)                     # the padded crop: offsets drawn on each image's own size
    t32 = pad.draw(4, np.array([33, 40, 32, 64]), np.array([35, 32, 50, 64]))
    rng = random.Random(3 * 65536)
    for b, (h0, w0) in enumerate(((33, 35), (40, 32), (32, 50), (64, 64))):
        y0, x0 = rng.randint(0, h0 + 8 - 32) - 4, rng.randint(0, w0 + 8 - 32) - 4
        flip = int(rng.random() < 0.5)
        assert (t32["y0"][b], t32["x0"][b], t32["flip"][b], t32["filter"][b]) == (y0, x0, flip, 0)
    ev = data.EvalTransform(48).draw(3, H[:3], W[:3])
    for b in range(3):
        assert (ev["Rh"][b], ev["Rw"][b], ev["oy"][b], ev["ox"][b]) == RM.eval_geometry(int(H[b]), int(W[b]), 48)
        assert (ev["h"][b], ev["w"][b], ev["filter"][b]) == (H[b], W[b], M.BICUBIC)


# ============================================================================================ the packed set
def _three_sizes():
    rng = np.random.RandomState(2)
    return [rng.randint(0, 256, s).astype(np.uint8) for s in ((20, 28, 3), (33, 35, 3), (61, 130, 3), (20, 28, 3), (5, 1, 3))]


def test_from_arrays_packs(gold):
    from devit_amd import _lib, data
    arrays = _three_sizes()
    s = data.DeviceImageSet.from_arrays(arrays, [0, 1, 2, 1, 0], ["a", "b", "c"], device="cpu", ragged=True)
    assert s.ragged and len(s) == 5 and s.images is None and s.sizes.dtype == np.int32 and s.sizes.tolist() == [list(a.shape[:2]) for a in arrays]
    assert s.labels.tolist() == [0, 1, 2, 1, 0] and s.classes == ["a", "b", "c"] and s.arena.dtype == torch.uint8 and s.arena.dim() == 1
    with pytest.raises(ValueError, match="one size per image"):
        s.size
    ent = s.entries.numpy().view(data.IMAGE_ENTRY_DTYPE)
    arena, model_entries = RM.pack(arrays)
    assert [tuple(int(v) for v in e) for e in ent] == model_entries and np.array_equal(s.arena.numpy(), arena)
    assert (ent["offset"] % 16 == 0).all() and s.entries.numel() == 5 * C.sizeof(_lib.ImageEntry)
    for e, a in zip(ent, arrays):
        assert np.array_equal(s.arena.numpy()[int(e["offset"]):int(e["offset"]) + a.size].reshape(a.shape), a)
    auto = data.DeviceImageSet.from_arrays(arrays, [0] * 5, device="cpu", ragged="auto")
    assert auto.ragged
    same = data.DeviceImageSet.from_arrays([arrays[0], arrays[3]], [0, 1], device="cpu", ragged="auto")
    assert not same.ragged and same.size == (20, 28) and tuple(same.images.shape) == (2, 20, 28, 3)
    forced = data.DeviceImageSet.from_arrays(np.stack([arrays[0], arrays[3]]), [0, 1], device="cpu", ragged=True)
    assert forced.ragged and forced.sizes.tolist() == [[20, 28], [20, 28]]
    with pytest.raises(ValueError, match="resident sets are uniform"):          # the default keeps its refusal
        data.DeviceImageSet.from_arrays(arrays, [0] * 5, device="cpu")
    with pytest.raises(ValueError, match="image 1 must be uint8"):
        data.DeviceImageSet.from_arrays([arrays[0], arrays[1].astype(np.float32)], [0, 1], device="cpu", ragged=True)


def test_directory_validation():
    from devit_amd import data
    arena, entries = data.pack_images(_three_sizes())
    data.check_directory(entries, arena.shape[0])
    for field, i, value, msg in (("H", 1, 0, "image 1 is 0 x 35"), ("W", 2, -3, "image 2 is 61 x -3"), ("offset", 4, arena.shape[0] - 8, "image 4 .* reaches past"),
                                 ("H", 2, 62, "overlap|reaches past"), ("offset", 1, 16, "images 0 and 1 overlap"), ("offset", 3, 2 ** 40, "reaches past")):
        bad = entries.copy()
        bad[field][i] = value
        with pytest.raises(ValueError, match=msg):
            data.check_directory(bad, arena.shape[0])
        with pytest.raises(ValueError, match=msg):
            data.DeviceImageSet.from_packed(arena, bad, [0] * 5, device="cpu")
    with pytest.raises(ValueError, match="IMAGE_ENTRY_DTYPE"):
        data.check_directory(entries.view(np.uint8), arena.shape[0])


def _tree(Image, root, sizes=((20, 28), (33, 35), (61, 130))):
    rng = np.random.RandomState(1)
    want = {}
    for ci, c in enumerate(("zebra", "ant", "bee")):
        (root / c).mkdir(parents=True)
        for k, fn in enumerate(("2.png", "10.png", "1.png")):
            a = rng.randint(0, 256, (*sizes[(ci + k) % len(sizes)], 3)).astype(np.uint8)
            Image.fromarray(a).save(root / c / fn)
            want[(c, fn)] = a
    return want


def test_from_folder_ragged(tmp_path, monkeypatch):
    Image = pytest.importorskip("PIL.Image")
    from devit_amd import data
    want = _tree(Image, tmp_path / "set")
    (tmp_path / "set" / "ant" / "notes.txt").write_text("not an image")
    s = data.DeviceImageSet.from_folder(str(tmp_path / "set"), device="cpu", ragged=True)
    order = [(c, fn) for c in ("ant", "bee", "zebra") for fn in ("1.png", "10.png", "2.png")]        # sorted as strings, like ImageFolder
    assert s.ragged and s.classes == ["ant", "bee", "zebra"] and s.labels.tolist() == [0] * 3 + [1] * 3 + [2] * 3
    assert s.sizes.tolist() == [list(want[k].shape[:2]) for k in order] and len({tuple(v) for v in s.sizes.tolist()}) == 3
    ent = s.entries.numpy().view(data.IMAGE_ENTRY_DTYPE)
    for e, k in zip(ent, order):
        a = want[k]
        assert (e["H"], e["W"]) == a.shape[:2] and e["offset"] % 16 == 0
        assert np.array_equal(s.arena.numpy()[int(e["offset"]):int(e["offset"]) + a.size].reshape(a.shape), a), k
    assert data.DeviceImageSet.from_folder(str(tmp_path / "set"), device="cpu", ragged="auto").ragged
    with pytest.raises(ValueError, match="resident sets are uniform"):          # the default keeps its refusal
        data.DeviceImageSet.from_folder(str(tmp_path / "set"), device="cpu")
    assert data.DECODE_WORKERS <= 16
    # the budget: refused from the headers, before anything is decoded
    total = int(sum((a.size + 15) // 16 * 16 for a in want.values()))
    data.DeviceImageSet.from_folder(str(tmp_path / "set"), device="cpu", ragged=True, budget_bytes=total)
    decoded = []
    monkeypatch.setattr(Image.Image, "convert", lambda self, *a, **k: decoded.append(1))
    with pytest.raises(SystemExit, match=rf"take {total} bytes .* budget .* is {total - 1} bytes .*largest image is .*61 x 130"):
        data.DeviceImageSet.from_folder(str(tmp_path / "set"), device="cpu", ragged=True, budget_bytes=total - 1)
    assert decoded == []


def test_auto_gives_the_uniform_form_on_a_uniform_tree(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    from devit_amd import data
    want = _tree(Image, tmp_path / "set", sizes=((20, 28),))
    s = data.DeviceImageSet.from_folder(str(tmp_path / "set"), device="cpu", ragged="auto")
    old = data.DeviceImageSet.from_folder(str(tmp_path / "set"), device="cpu")
    assert not s.ragged and s.size == (20, 28) and torch.equal(s.images, old.images) and torch.equal(s.labels, old.labels) and s.classes == old.classes
    assert np.array_equal(s.images[1].numpy(), want[("ant", "10.png")])


def test_save_load_round_trip(tmp_path):
    from devit_amd import data
    arrays = _three_sizes()
    s = data.DeviceImageSet.from_arrays(arrays, [0, 1, 2, 1, 0], ["a", "b b", "c"], device="cpu", ragged=True)
    assert not data.DeviceImageSet.saved(str(tmp_path / "p"))
    s.save(str(tmp_path / "p"))
    assert data.DeviceImageSet.saved(str(tmp_path / "p")) and sorted(os.listdir(tmp_path / "p")) == ["arena.npy", "classes.npy", "entries.npy", "labels.npy"]
    t = data.DeviceImageSet.load(str(tmp_path / "p"), device="cpu")
    assert t.ragged and torch.equal(t.arena, s.arena) and torch.equal(t.entries, s.entries) and torch.equal(t.labels, s.labels)
    assert t.classes == s.classes and np.array_equal(t.sizes, s.sizes)
    u = data.DeviceImageSet.from_arrays(np.stack([arrays[0], arrays[3]]), [1, 0], device="cpu")
    u.save(str(tmp_path / "u"))
    v = data.DeviceImageSet.load(str(tmp_path / "u"), device="cpu")
    assert not v.ragged and torch.equal(v.images, u.images) and v.labels.tolist() == [1, 0] and v.classes == ["0", "1"]
    bad = np.load(tmp_path / "p" / "entries.npy")
    bad["H"][2] = 4000
    np.save(tmp_path / "p" / "entries.npy", bad)
    with pytest.raises(ValueError, match="reaches past"):                        # a loaded directory is validated like any other
        data.DeviceImageSet.load(str(tmp_path / "p"), device="cpu")


# ============================================================================================ refusals, tables, the loader's state
def _sparse_set(sizes):
    """a packed set of zero images of the given sizes, built without materialising more than the arena"""
    from devit_amd import data
    return data.DeviceImageSet.from_arrays([np.zeros((h, w, 3), np.uint8) for h, w in sizes], list(range(len(sizes))), device="cpu", ragged=True)


def test_check_set_names_the_over_wide_images():
    from devit_amd import data
    H, W = np.array([100, 1600, 40, 1700, 1537]), np.array([100, 30, 1560, 1700, 20])
    data.TrainAugment(48).check_set(np.array([100, 1536, 40]), np.array([100, 30, 1536]))          # 1536 / 48 * 4 = 128 taps: served
    with pytest.raises(ValueError, match=r"4 image\(s\) .* more than 128 taps .*image 1 \(1600 x 30: 13\d taps\), image 2 \(40 x 1560: 13\d taps\), image 3"):
        data.TrainAugment(48).check_set(H, W)
    data.TrainAugment(224).check_set(H, W)
    data.TrainAugment(48, interpolation='bilinear').check_set(H, W)                               # half the support
    with pytest.raises(ValueError, match="image 1 "):
        data.TrainAugment(48, interpolation='random').check_set(H, W)
    data.EvalTransform(48).check_set(np.array([100, 1600]), np.array([100, 30]))                    # the short side to 54: 1600 -> 2880, up-scaling
    with pytest.raises(ValueError, match=r"EvalTransform at 48 pixels: 1 image.*image 1 \(1800 x 1750"):
        data.EvalTransform(48).check_set(np.array([100, 1800]), np.array([100, 1750]))
    with pytest.raises(ValueError, match="padded 32 x 32 crop does not fit image 1 \\(23 x 40\\)"):
        data.TrainAugment(32).check_set(np.array([33, 23]), np.array([35, 40]))
    with pytest.raises(ValueError, match="as they are, and image 0 is 33 x 35"):
        data.EvalTransform(32).check_set(np.array([33]), np.array([35]))
    # a uniform set keeps the 12-tap refusal and its wording; a packed one of the same images is served
    with pytest.raises(ValueError, match="needs 14 taps .* holds 12"):
        data.TrainAugment(48).check_set(160, 160)
    s = _sparse_set([(160, 160), (20, 28)])
    ld = data.DeviceLoader(s, range(2), 2, data.TrainAugment(48), drop_last=True)
    assert len(ld) == 1
    with pytest.raises(ValueError, match="image 1 \\(1600 x 8"):
        data.DeviceLoader(_sparse_set([(20, 28), (1600, 8)]), range(2), 2, data.TrainAugment(48), drop_last=True)


def test_check_table_ragged_returns_max_taps():
    from devit_amd import data
    H, W = np.array([20, 200, 61, 146, 40]), np.array([28, 61, 330, 145, 700])
    tab = data.EvalTransform(48).draw(5, H, W)
    tab["Rh"], tab["Rw"], tab["oy"], tab["ox"] = 48, 48, 0, 0                  # every image whole to 48 x 48
    want = max(RM.taps_bound(int(n), 48, M.BICUBIC) for n in (200, 330, 146, 700))
    assert data.check_table(tab, H, W, 48) == want == RM.max_taps([M.row(0, 0, int(h), int(w), 48) for h, w in zip(H, W)])
    assert data.check_table(tab[:1], H[:1], W[:1], 48) == 5 and data.check_table(tab[3:4], H[3:4], W[3:4], 48) in (13, 14)
    assert data.check_table(data.TrainAugment(32, seed=1).draw(5, H + 20, W + 20), H + 20, W + 20, 32) == 1
    assert data.check_table(tab[:1], 20, 28, 48) is None                       # ints: the uniform form, as before
    for field, b, value, msg in (("h", 1, 201, "inside its image"), ("x0", 2, 1, "inside its image"), ("filter", 0, 3, "filter"), ("h", 4, 0, "empty"),
                                 ("Rw", 3, 40, "window")):
        bad = tab.copy()
        bad[field][b] = value
        with pytest.raises(ValueError, match=msg):
            data.check_table(bad, H, W, 48)
    big = tab[:1].copy()
    big["h"], big["w"] = 1537, 28
    with pytest.raises(ValueError, match="row 0 .* needs 129 taps .* holds 128"):
        data.check_table(big, np.array([1537]), np.array([28]), 48)
    with pytest.raises(ValueError, match="2 image sizes for a table of 5 rows"):
        data.check_table(tab, H[:2], W[:2], 48)


def test_ragged_loader_state_round_trip():
    from devit_amd import data
    s = _sparse_set([(20, 28), (33, 35), (61, 130), (200, 61)])
    kw = dict(interpolation='random', re_prob=0.5, re_mode='rand', re_count=2, seed=6)
    a = data.DeviceLoader(s, range(4), 2, data.TrainAugment(48, **kw), drop_last=True)
    a.transform.draw(3, s.sizes[[0, 2, 3], 0], s.sizes[[0, 2, 3], 1])
    state = a.transform.state_dict()
    b = data.DeviceLoader(s, range(4), 2, data.TrainAugment(48, **kw), drop_last=True)
    b.transform.load_state_dict(state)
    idx = [3, 1, 1, 0]
    assert a.transform.draw(4, s.sizes[idx, 0], s.sizes[idx, 1]).tobytes() == b.transform.draw(4, s.sizes[idx, 0], s.sizes[idx, 1]).tobytes()
    assert b.transform.drawn == 7


# ============================================================================================ the CLI paths
def _args(argv):
    import distill_sub
    return argparse.ArgumentParser(parents=[distill_sub.get_args_parser()]).parse_args(argv)


OK = ["--device-data", "--aa", "none", "--color-jitter", "0", "--input-size", "48", "--batch-size", "2", "--eval-batch-size", "2"]


def test_cli_imnet_cache_and_named_refusals(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    import distill_sub
    _tree(Image, tmp_path / "imnet" / "train")
    _tree(Image, tmp_path / "imnet" / "val", sizes=((33, 35),))
    argv = OK + ["--dataset", "IMNET", "--data-path", str(tmp_path / "imnet")]
    tr, va, nc = distill_sub.build_loaders(_args(argv), 1000, "cpu", provider="whole", plain_sampler_over="train")
    assert nc == 3 and tr.dataset.ragged and len(tr.dataset) == 9 and not va.dataset.ragged and va.dataset.size == (33, 35) and len(va) == 5
    for name, why in (("flowers", r"\.mat"), ("cars", r"\.mat"), ("pets", "annotation list"), ("INAT", "json"), ("INAT19", "json")):
        with pytest.raises(SystemExit, match=f"--dataset {name}: .*{why}") as e:
            args = _args(OK)
            args.dataset = name                        # (INAT and INAT19 are not among the parser's choices; build_dataset knows them)
            distill_sub.build_loaders(args, 10, "cpu", provider="whole", plain_sampler_over="train")
        assert "mixed sizes" not in str(e.value)
    # --device-data-cache: written on the first run, loaded on the second (the folders may be gone by then)
    cache = tmp_path / "cache"
    tr1, va1, _ = distill_sub.build_loaders(_args(argv + ["--device-data-cache", str(cache)]), 1000, "cpu", provider="whole", plain_sampler_over="train")
    assert sorted(os.listdir(cache)) == ["test", "train"] and "arena.npy" in os.listdir(cache / "train") and "images.npy" in os.listdir(cache / "test")
    gone = OK + ["--dataset", "IMNET", "--data-path", str(tmp_path / "nowhere"), "--device-data-cache", str(cache)]
    tr2, va2, nc2 = distill_sub.build_loaders(_args(gone), 1000, "cpu", provider="whole", plain_sampler_over="train")
    assert nc2 == 3 and torch.equal(tr2.dataset.arena, tr1.dataset.arena) and torch.equal(tr2.dataset.entries, tr.dataset.entries)
    assert torch.equal(va2.dataset.images, va.dataset.images) and tr2.dataset.classes == ["ant", "bee", "zebra"]
    with pytest.raises(SystemExit, match="not a directory"):
        distill_sub.build_loaders(_args(gone[:-2]), 1000, "cpu", provider="whole", plain_sampler_over="train")
    for script in ("train_subdata.py", "ensemble.py"):                                    # the flags reach the other two CLIs
        assert "ds.get_args_parser()" in open(os.path.join(ROOT, script)).read()


def test_cli_division_tree_of_mixed_sizes(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    import distill_sub
    _tree(Image, tmp_path / "sub-dataset2" / "train_dataset")
    _tree(Image, tmp_path / "sub-dataset2" / "test_dataset")
    tr, va, nc = distill_sub.build_loaders(_args(OK + ["--data-path", str(tmp_path), "--start-division", "2", "--no-repeated-aug"]), 25, "cpu", provider="division")
    assert nc == 3 and tr.dataset.ragged and va.dataset.ragged and len(va) == 5 and tr.drop_last and not va.drop_last


# ============================================================================================ ABI
def test_image_entry_layout():
    """header struct, ctypes mirror and numpy mirror of devit_image_entry agree field by field (test_abi.py holds symbols, count and sizeof)"""
    from devit_amd import _lib, data
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "devit_hip.h")).read(), flags=re.S)
    end = src.index("} devit_image_entry;")
    body = src[src.rindex("typedef struct {", 0, end) + len("typedef struct {"):end]
    names = []
    for stmt in body.split(";"):
        for piece in stmt.split(","):
            ids = re.findall(r"[A-Za-z_][A-Za-z0-9_]*", piece)
            if ids:
                names.append(ids[-1])
    assert names == [f[0] for f in _lib.ImageEntry._fields_] == list(data.IMAGE_ENTRY_DTYPE.names) == ["offset", "H", "W"]
    assert C.sizeof(_lib.ImageEntry) == data.IMAGE_ENTRY_DTYPE.itemsize == 16
    for n in names:
        assert getattr(_lib.ImageEntry, n).offset == data.IMAGE_ENTRY_DTYPE.fields[n][1], n
    assert _lib.ABI_STRUCTS[16] is _lib.ImageEntry and {"devit_augment_ragged", "devit_augment_ragged_workspace"} <= set(_lib.SIGNATURES)
    for macro, value in (("DEVIT_AUGMENT_TAPS_MAX", 128), ("DEVIT_AUGMENT_FORCE_WIDE", 1), ("DEVIT_AUGMENT_TAPS", 12)):
        assert int(re.search(r"#define %s (\w+)" % macro, src).group(1).rstrip("u"), 0) == value
