"""Host side of the image-op layers (include/devit_hip.h "Image ops"; devit_amd/data.py): the numpy restatement (tests/_randaug_model.py) against
PIL -- the committed golden, and PIL live where it imports, 224 x 224 included --, against planted bugs, the draws of TrainAugment against the
independent restatement, the config parser, the CLI with and without --device-aug, and the struct layout.  Nothing here needs a GPU."""
import argparse
import ctypes as C
import math
import os
import random
import re

import numpy as np
import pytest

import _randaug_model as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "randaug_pil.npz")))


# ============================================================================================ the ops against PIL
def test_model_equals_the_golden(gold):
    cases = R.golden_cases(gold)
    assert len(cases) >= 140
    seen, chains = {}, set()
    for i, (img, layers, px) in enumerate(cases):
        assert np.array_equal(R.apply_layers(img, layers), px), (i, [(L["op"], L["filter"], L["factor"], L["arg"]) for L in layers])
        chains.add(len(layers))
        for L in layers:
            seen.setdefault(L["op"], []).append(L)
    assert set(seen) == set(range(15)) and chains >= {1, 2, 3, 4}
    # the extremes the kernels are held to are in the file
    assert {L["arg"] for L in seen[R.POSTERIZE]} >= {0, 4} and {L["arg"] for L in seen[R.SOLARIZE]} >= {0, 256}
    for op in (R.COLOR, R.CONTRAST, R.BRIGHTNESS, R.SHARPNESS):
        assert {round(L["factor"], 2) for L in seen[op]} >= {0.1, 1.0, 1.9}
    for op in R.AFFINE_OPS:
        assert {L["filter"] for L in seen[op]} == {R.BILINEAR, R.BICUBIC}
    assert any(L["matrix"] == R.IDENTITY for L in seen[R.ROTATE]) and any(abs(L["matrix"][2]) >= 32 for L in seen[R.TRANSLATE_X])
    assert {np.sign(L["matrix"][1]) for L in seen[R.SHEAR_X]} >= {-1.0, 1.0}
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "randaug_pil.npz")) < 1 << 20


def _pil_apply(img, L, S):
    from PIL import Image, ImageEnhance, ImageOps
    op, kw = L["op"], dict(resample={1: Image.BILINEAR, 2: Image.BICUBIC}[L["filter"]], fillcolor=L["fill"])
    if op == R.AUTOCONTRAST:
        return ImageOps.autocontrast(img)
    if op == R.EQUALIZE:
        return ImageOps.equalize(img)
    if op == R.INVERT:
        return ImageOps.invert(img)
    if op == R.POSTERIZE:
        return ImageOps.posterize(img, L["arg"])
    if op == R.SOLARIZE:
        return ImageOps.solarize(img, L["arg"])
    if op == R.SOLARIZE_ADD:
        lut = [min(255, i + L["arg"]) if i < 128 else i for i in range(256)]
        return img.point(lut * 3)
    if op in (R.COLOR, R.CONTRAST, R.BRIGHTNESS, R.SHARPNESS):
        return {R.COLOR: ImageEnhance.Color, R.CONTRAST: ImageEnhance.Contrast, R.BRIGHTNESS: ImageEnhance.Brightness,
                R.SHARPNESS: ImageEnhance.Sharpness}[op](img).enhance(L["factor"])
    if op == R.ROTATE:
        return img.rotate(L["deg"], **kw)
    return img.transform(img.size, Image.AFFINE, L["matrix"], **kw)


def _random_layer(rng, S):
    op = int(rng.randint(15))
    filt = int(rng.randint(1, 3))
    if op == R.ROTATE:
        deg = float(rng.uniform(-30, 30))
        return dict(R.layer(op, filt, matrix=R.rotate_matrix(deg, S)), deg=deg)
    if op in R.AFFINE_OPS:
        v = float(rng.uniform(-0.3, 0.3)) if op in (R.SHEAR_X, R.SHEAR_Y) else float(rng.uniform(-0.45, 0.45)) * S
        return R.layer(op, filt, matrix=R.affine_matrix(op, v, S))
    if op in (R.COLOR, R.CONTRAST, R.BRIGHTNESS, R.SHARPNESS):
        return R.layer(op, factor=float(rng.uniform(0.1, 1.9)))
    return R.layer(op, arg=int({R.POSTERIZE: rng.randint(0, 5), R.SOLARIZE: rng.randint(0, 257), R.SOLARIZE_ADD: rng.randint(0, 111)}.get(op, 0)))


def test_model_equals_pil_live():
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.RandomState(3)
    n, ops_seen = 0, set()
    for S, count in ((32, 150), (48, 60), (224, 16)):
        for i in range(count):
            img = rng.randint(0, 256, (S, S, 3)).astype(np.uint8)
            if i % 3 == 0:                                  # smooth content with saturated blocks: the cubic overshoots at both ends
                y, x = np.mgrid[0:S, 0:S]
                img = np.clip(128 + 120 * np.sin((y * 2 + x * 3) / 9.0)[:, :, None] * np.array([1.0, -0.8, 0.5]) + rng.randint(-20, 21, (S, S, 3)), 0, 255).astype(np.uint8)
                img[S // 4:S // 2, S // 3:S // 2] = 255 * (i % 2)
            layers = [_random_layer(rng, S) for _ in range(1 if S == 224 else int(rng.randint(1, 4)))]
            pil = Image.fromarray(img)
            for L in layers:
                pil = _pil_apply(pil, L, S)
            assert np.array_equal(R.apply_layers(img, layers), np.asarray(pil)), (S, i, [(L["op"], L["filter"], L["factor"], L["arg"], L["matrix"]) for L in layers])
            ops_seen |= {L["op"] for L in layers}
            n += 1
    # the expensive ones at 224 explicitly: a non-trivial bicubic rotation, Equalize, Sharpness, Contrast
    img = rng.randint(0, 256, (224, 224, 3)).astype(np.uint8)
    layers = [dict(R.layer(R.ROTATE, R.BICUBIC, matrix=R.rotate_matrix(-23.5, 224)), deg=-23.5), R.layer(R.EQUALIZE), R.layer(R.SHARPNESS, factor=1.7),
              R.layer(R.CONTRAST, factor=0.35)]
    pil = Image.fromarray(img)
    for L in layers:
        pil = _pil_apply(pil, L, 224)
    assert np.array_equal(R.apply_layers(img, layers), np.asarray(pil))
    assert n == 226 and ops_seen == set(range(15))


@pytest.mark.parametrize("bug,layers", [
    ("blend_double", [R.layer(R.BRIGHTNESS, factor=1.3)]), ("blend_fma", [R.layer(R.COLOR, factor=1.6)]), ("blend_round", [R.layer(R.BRIGHTNESS, factor=0.73)]),
    ("cubic_no_clamp", [R.layer(R.SHEAR_X, R.BICUBIC, matrix=R.affine_matrix(R.SHEAR_X, 0.21, 48))]), ("smooth_border", [R.layer(R.SHARPNESS, factor=1.8)]),
    ("contrast_mean_floor", [R.layer(R.CONTRAST, factor=0.2)]),
    ("fill_on_clamped_edges", [R.layer(R.TRANSLATE_X, R.BILINEAR, matrix=R.affine_matrix(R.TRANSLATE_X, 0.25, 48))]),
    ("layers_reversed", [R.layer(R.SOLARIZE, arg=100), R.layer(R.BRIGHTNESS, factor=1.5)])])
def test_golden_catches_planted_bugs(gold, bug, layers):
    """each planted bug changes bytes on the golden's own sources (so the comparison with PIL's bytes above would fail for it)"""
    hit = 0
    for img in list(gold["src48"]) + list(gold["src32"][:4]):
        if layers[0]["op"] in R.AFFINE_OPS and img.shape[0] != 48:
            continue
        hit += int((R.apply_layers(img, layers, bug=bug) != R.apply_layers(img, layers)).sum())
    if bug == "contrast_mean_floor":      # the mean's fraction must lie above one half somewhere: look over the sources' rolls too
        for img in gold["src32"][:4]:
            for k in range(1, 8):
                im = np.clip(img.astype(int) + k, 0, 255).astype(np.uint8)
                hit += int((R.apply_layers(im, layers, bug=bug) != R.apply_layers(im, layers)).sum())
    assert hit > 0, bug


# ============================================================================================ the draws
def _layers_of(t):
    return [R.layer(int(t["op"][k]), int(t["filter"][k]), float(t["factor"][k]), int(t["arg"][k]), tuple(t["matrix"][k]), tuple(int(v) for v in t["fill"][k][:3]))
            for k in range(int(t["n_ops"]))]


def _same(a, b):
    """a drawn table layer against a restated one: the factor is stored as fp32"""
    return (a["op"], a["filter"], a["arg"], a["matrix"], a["fill"]) == (b["op"], b["filter"], b["arg"], b["matrix"], b["fill"]) and \
        a["factor"] == float(np.float32(b["factor"]))


@pytest.mark.parametrize("S,kw", [(48, dict(auto_augment="rand-m9-mstd0.5-inc1")), (224, dict(auto_augment="rand-m7-n3-mstd1.5-inc1", interpolation="random")),
                                  (64, dict(auto_augment="rand-m10-inc1", interpolation="bilinear")), (32, dict(auto_augment="rand-m9-mstdinf-inc1-n4")),
                                  (48, dict(color_jitter=0.4, interpolation="random"))])
def test_draws_equal_the_restatement(S, kw):
    from devit_amd import data
    seed, rank, B, H0, W0 = 5, 2, 29, 32, 32
    common = dict(re_prob=0.5, re_mode="pixel", re_count=2, seed=seed, rank=rank)
    tf = data.TrainAugment(S, **common, **kw)
    twin = data.TrainAugment(S, **common, interpolation=kw.get("interpolation", "bicubic"))      # the parent's draws: crop, filter, flip, erase
    rng = random.Random(seed * 65536 + rank)
    m, n, mstd = R.parse_rand(kw["auto_augment"]) if "auto_augment" in kw else (0, 0, 0.0)
    fill = R.fill_colour(data.IMAGENET_DEFAULT_MEAN)
    assert fill == (124, 116, 104)
    interp = kw.get("interpolation", "bicubic")
    applied = 0
    for _ in range(2):
        tab, lay = tf.draw_with_ops(B, H0, W0)
        data.check_ops_table(lay, B)
        data.check_table(tab, H0, W0, S)
        for b in range(B):
            # one sample of the parent's stream on the shared generator, with the layers between its flip and its erase draws
            twin.rng = rng
            if S == 32:
                box = (rng.randint(0, H0 + 8 - S) - 4, rng.randint(0, W0 + 8 - S) - 4, S, S)
                filt = 0
            else:
                box = twin._crop(H0, W0)
                filt = rng.choice((1, 2)) if interp == "random" else {"bilinear": 1, "bicubic": 2}[interp]
            flip = int(rng.random() < 0.5)
            want = R.draw_rand_layers(rng, S, m, n, mstd, interp, fill) if "auto_augment" in kw else R.draw_jitter_layers(rng, kw["color_jitter"], fill)
            boxes = twin._erase()
            t = tab[b]
            assert (int(t["y0"]), int(t["x0"]), int(t["h"]), int(t["w"]), int(t["filter"]), int(t["flip"]), int(t["n_erase"])) == (*box, filt, flip, len(boxes)), b
            got = _layers_of(lay[b])
            assert len(got) == len(want) and all(_same(g, w) for g, w in zip(got, want)), (b, got, want)
            applied += len(got)
    assert applied > B // 2
    with pytest.raises(ValueError, match="draw_with_ops"):
        tf.draw(B, H0, W0)


def test_both_off_is_the_parent_stream():
    from devit_amd import data
    kw = dict(interpolation="random", re_prob=0.5, re_mode="rand", re_count=3, seed=9, rank=1)
    a, b = data.TrainAugment(48, **kw), data.TrainAugment(48, auto_augment=None, color_jitter=0.0, **kw)
    c = data.TrainAugment(48, auto_augment="none", color_jitter=None, **kw)
    want = a.draw(40, 32, 32)
    tab, lay = b.draw_with_ops(40, 32, 32)
    assert lay is None and tab.tobytes() == want.tobytes() == c.draw(40, 32, 32).tobytes()
    assert set(a.state_dict()) == {"rng", "drawn"} == set(data.TrainAugment(48, auto_augment="rand-m9-inc1").state_dict())
    # the layers' draws travel with the generator's state (gauss's spare value included)
    d = data.TrainAugment(48, auto_augment="rand-m9-mstd0.5-inc1", seed=2)
    d.draw_with_ops(7, 32, 32)
    state = d.state_dict()
    want = d.draw_with_ops(9, 32, 32)
    e = data.TrainAugment(48, auto_augment="rand-m9-mstd0.5-inc1", seed=2)
    e.load_state_dict(state)
    got = e.draw_with_ops(9, 32, 32)
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
    # with auto_augment set, ColorJitter is not applied (timm: if auto_augment ... elif color_jitter)
    f = data.TrainAugment(48, auto_augment="rand-m9-mstd0.5-inc1", color_jitter=0.4, seed=2)
    assert f.color_jitter == 0.0 and f.draw_with_ops(7, 32, 32)[1].tobytes() == data.TrainAugment(48, auto_augment="rand-m9-mstd0.5-inc1", seed=2).draw_with_ops(7, 32, 32)[1].tobytes()


def test_op_and_apply_shares():
    """20 000 seeded draws: each op's share within 4 standard deviations of 1 / 15, the applied share within 4 of 1 / 2"""
    from devit_amd import data
    tf = data.TrainAugment(48, auto_augment="rand-m9-mstd0.5-inc1-n1", seed=11)
    N = 20000
    _, lay = tf.draw_with_ops(N, 32, 32)
    applied = int(lay["n_ops"].sum())
    assert abs(applied - N / 2) <= 4 * math.sqrt(N * 0.25), applied
    counts = np.bincount(lay["op"][lay["n_ops"] == 1, 0], minlength=15)
    p = 1 / 15
    assert (np.abs(counts - applied * p) <= 4 * math.sqrt(applied * p * (1 - p))).all(), counts


# ============================================================================================ parser, validation, CLI
def test_parser():
    from devit_amd import data
    assert data.parse_auto_augment("rand-m9-mstd0.5-inc1") == {"m": 9, "n": 2, "mstd": 0.5}
    assert data.parse_auto_augment("rand-inc1-n3") == {"m": 10, "n": 3, "mstd": 0.0}
    assert data.parse_auto_augment("rand-m4-mstdinf-inc1")["mstd"] == float("inf")
    for config, msg in (("rand-m9-mstd0.5", "inc0"), ("rand-m9-inc0", "inc0"), ("rand-m9-inc1-w0", "weighted"), ("augmix-m3-w3", "AugMix"),
                        ("original", "AutoAugment"), ("v0", "AutoAugment"), ("rand-m9-inc1-n5", "1 .. 4 layers"), ("rand-m9-inc1-n0", "1 .. 4 layers"),
                        ("rand-mx-inc1", "does not parse"), ("rand-m9-inc1-p0.3", "unknown section")):
        with pytest.raises(ValueError, match=msg):
            data.parse_auto_augment(config)
    with pytest.raises(ValueError, match="inc0"):
        data.TrainAugment(48, auto_augment="rand-m9-mstd0.5")
    with pytest.raises(ValueError, match="negative"):
        data.TrainAugment(48, color_jitter=-0.1)


def test_ops_table_validation():
    from devit_amd import data
    _, good = data.TrainAugment(48, auto_augment="rand-m9-mstd0.5-inc1-n4", seed=1).draw_with_ops(64, 32, 32)
    data.check_ops_table(good, 64)
    b = int(np.nonzero((good["n_ops"] > 0) & np.isin(good["op"][:, 0], R.AFFINE_OPS))[0][0])
    for field, value, msg in (("n_ops", 5, "n_ops"), ("n_ops", -1, "n_ops"), ("op", 15, "op ids"), ("filter", 0, "filter"), ("matrix", np.nan, "finite"),
                              ("matrix", np.inf, "finite"), ("factor", np.nan, "finite"), ("fill", 256, "fill")):
        bad = good.copy()
        if field == "n_ops":
            bad[field][b] = value
        else:
            bad[field][b][0] = value
        with pytest.raises(ValueError, match=msg):
            data.check_ops_table(bad, 64)
    with pytest.raises(ValueError, match="64"):
        data.check_ops_table(good[:5], 64)


def _args(argv):
    import distill_sub
    return argparse.ArgumentParser(parents=[distill_sub.get_args_parser()]).parse_args(argv)


def test_cli_with_and_without_device_aug(tmp_path):
    import distill_sub
    base = ["--device-data", "--input-size", "48"]
    for extra in ([], ["--aa", "rand-m5-inc1-n3"], ["--color-jitter", "0.2", "--aa", "none"], ["--no_aug"], ["--aa", "none", "--color-jitter", "0"]):
        distill_sub.check_device_data(_args(base + ["--device-aug"] + extra))                 # the defaults (RandAugment + ColorJitter 0.4) included
    for extra, msg in ((["--aa", "rand-m9-mstd0.5"], "inc0"), (["--aa", "augmix-m3"], "AugMix"), (["--aa", "rand-m9-inc1-n7"], "layers"),
                       (["--synthetic", "2"], "--synthetic"), (["--recount", "5"], "--recount 5")):
        with pytest.raises(SystemExit, match=msg):
            distill_sub.check_device_data(_args(base + ["--device-aug"] + extra))
    with pytest.raises(SystemExit, match="--device-data"):
        distill_sub.check_device_data(_args(["--device-aug"]))
    for extra, msg in ((["--aa", "rand-m9-mstd0.5-inc1", "--color-jitter", "0"], "RandAugment.*--device-aug"), (["--aa", "none", "--color-jitter", "0.4"], "ColorJitter.*--device-aug"),
                       (["--aa", "none", "--color-jitter", "0", "--no_aug"], "--no_aug.*--device-aug")):
        with pytest.raises(SystemExit, match=msg):
            distill_sub.check_device_data(_args(base + extra))
    for script in ("train_subdata.py", "ensemble.py"):
        assert "ds.get_args_parser()" in open(os.path.join(ROOT, script)).read()
    # the transform the loaders get
    Image = pytest.importorskip("PIL.Image")
    for split in ("train_dataset", "test_dataset"):
        for c in ("a", "b"):
            (tmp_path / "sub-dataset1" / split / c).mkdir(parents=True)
            for i in range(3):
                Image.fromarray(np.full((32, 32, 3), i, np.uint8)).save(tmp_path / "sub-dataset1" / split / c / f"{i}.png")
    common = base + ["--data-path", str(tmp_path), "--start-division", "1", "--batch-size", "2", "--no-repeated-aug", "--reprob", "0.25"]
    tf = distill_sub.build_loaders(_args(common + ["--device-aug"]), 25, "cpu", provider="division")[0].transform
    assert tf.rand == {"m": 9, "n": 2, "mstd": 0.5} and tf.color_jitter == 0.0 and tf.re_prob == 0.25 and tf.has_ops
    tf = distill_sub.build_loaders(_args(common + ["--device-aug", "--aa", "none"]), 25, "cpu", provider="division")[0].transform
    assert tf.rand is None and tf.color_jitter == 0.4
    tf = distill_sub.build_loaders(_args(common + ["--device-aug", "--no_aug"]), 25, "cpu", provider="division")[0].transform
    assert tf.rand is None and tf.color_jitter == 0.4 and tf.interpolation == "bilinear" and tf.re_prob == 0.0
    tf = distill_sub.build_loaders(_args(common + ["--aa", "none", "--color-jitter", "0"]), 25, "cpu", provider="division")[0].transform
    assert not tf.has_ops


# ============================================================================================ ABI
def test_ops_struct_layout():
    """header struct, ctypes mirror and numpy mirror of devit_augment_ops agree field by field; the op ids are the header's"""
    from devit_amd import _lib, data
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "devit_hip.h")).read(), flags=re.S)
    end = src.index("} devit_augment_ops;")
    body = src[src.rindex("typedef struct {", 0, end) + len("typedef struct {"):end]
    names = []
    for stmt in body.split(";"):
        ids = re.findall(r"[A-Za-z_][A-Za-z0-9_]*", re.sub(r"\[.*", "", stmt))
        if ids:
            names.append(ids[-1])
    assert names == [f[0] for f in _lib.AugmentOps._fields_] == list(data.AUG_OPS_DTYPE.names)
    assert C.sizeof(_lib.AugmentOps) == data.AUG_OPS_DTYPE.itemsize == 328
    for n in names:
        assert getattr(_lib.AugmentOps, n).offset == data.AUG_OPS_DTYPE.fields[n][1], n
    assert _lib.ABI_STRUCTS[15] is _lib.AugmentOps and {"devit_image_ops", "devit_augment_batch_ops", "devit_augment_ops_workspace"} <= set(_lib.SIGNATURES)
    assert C.sizeof(_lib.AugmentSample) == 120                                          # untouched
    enum = re.search(r"enum devit_image_op \{(.*?)\};", src, re.S).group(1)
    ids = {k: int(v) for k, v in re.findall(r"DEVIT_OP_(\w+) = (\d+)", enum)}
    assert ids.pop("COUNT") == 15 == _lib.OP_COUNT == R.N_OPS
    for k, v in ids.items():
        assert getattr(_lib, "OP_" + k) == v == getattr(R, k), k
    assert int(re.search(r"#define DEVIT_AUGMENT_MAX_OPS (\d+)", src).group(1)) == 4 == _lib.AUGMENT_MAX_OPS == R.MAX_OPS
