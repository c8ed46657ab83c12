"""The image-op layers on the device (csrc/augment.hip: devit_image_ops, devit_augment_batch_ops; include/devit_hip.h "Image ops") against PIL's own
bytes (tests/golden/randaug_pil.npz; PIL is not imported for them) and against tests/_randaug_model.py, byte for byte; the full stage (layers, then
normalize and erase) against model o tests/_augment_model.py within the normalization bound that file derives; memory safety for any table bytes;
DeviceLoader with auto_augment against the host-side composition of its own drawn tables; distill_sub.py --device-data --device-aug end to end."""
import argparse
import json
import os

import numpy as np
import pytest
import torch

import _augment_model as M
import _randaug_model as R
from conftest import chk

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
SENTINEL, GUARD = 12345.0, 64


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from devit_amd import _lib
    _lib.require_device(torch.zeros(1, device="cuda"))
    return torch.device("cuda")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "randaug_pil.npz")))


@pytest.fixture(scope="module")
def gold_aug():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "augment_pil.npz")))


def to_ops(samples):
    """[[layers] per sample] -> AUG_OPS_DTYPE [B]"""
    from devit_amd import data
    tab = np.zeros(len(samples), dtype=data.AUG_OPS_DTYPE)
    for t, layers in zip(tab, samples):
        t["n_ops"] = len(layers)
        for k, L in enumerate(layers):
            t["op"][k], t["filter"][k], t["factor"][k], t["arg"][k] = L["op"], L["filter"], L["factor"], L["arg"]
            t["matrix"][k] = L["matrix"]
            t["fill"][k][:3] = L["fill"]
    return tab


def run_ops(dev, images, samples):
    """devit_image_ops on uint8 [B][S][S][3] with sentinel bytes around the output -> uint8 [B][S][S][3] on the host"""
    from devit_amd import _lib, data, ops
    imgs = torch.from_numpy(np.ascontiguousarray(images)).to(dev)
    B, S = imgs.shape[0], imgs.shape[1]
    n = B * S * S * 3
    flat = torch.full((GUARD + n + S * S * 3 + GUARD,), 0xA5, dtype=torch.uint8, device=dev)       # one spare image behind B
    tab = to_ops(samples)
    data.check_ops_table(tab, B)
    tab_dev = data.upload(tab.view(np.uint8).reshape(-1), dev)
    ops.call("devit_image_ops", _lib.ptr(imgs), _lib.ptr(tab_dev), B, S, _lib.ptr(flat[GUARD:]), _lib.stream_ptr())
    got = flat.cpu().numpy()
    assert (got[:GUARD] == 0xA5).all() and (got[GUARD + n:] == 0xA5).all(), "wrote outside images 0 .. B-1 of out"
    assert np.array_equal(imgs.cpu().numpy(), images)                                               # the input is left alone
    return got[GUARD:GUARD + n].reshape(B, S, S, 3)


# ============================================================================================ PIL's bytes
def test_golden_cases(dev, gold):
    cases = R.golden_cases(gold)
    groups = {}
    for img, layers, px in cases:
        groups.setdefault(img.shape[0], []).append((img, layers, px))
    total, sizes, ops_seen = 0, set(), set()
    for S, group in sorted(groups.items()):
        at, B = 0, 1
        while at < len(group):                              # batches of 1, 2, .. 5, 1, ..: mixed ops and layer counts per batch
            part = group[at:at + B]
            got = run_ops(dev, np.stack([img for img, _, _ in part]), [layers for _, layers, _ in part])
            for b, (_, layers, px) in enumerate(part):
                diff = int((got[b] != px).sum())
                assert chk(diff, 1), (S, [(L["op"], L["filter"], L["factor"], L["arg"]) for L in layers], diff)
                ops_seen |= {L["op"] for L in layers}
            total += len(part)
            sizes.add(len(part))
            at, B = at + B, B % 5 + 1
    assert total == len(cases) and sizes >= {1, 2, 3, 4, 5} and ops_seen == set(range(15))


# ============================================================================================ the model at the largest and smallest sizes
def _big(S, seed):
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[0:S, 0:S]
    base = 128 + 100 * np.sin((y * 3 + x * 2) / 17.0)[:, :, None] * np.array([1.0, -0.7, 0.4])
    img = np.clip(base + rng.randint(-40, 41, (S, S, 3)), 0, 255)
    img[S // 4:S // 2, S // 3:S // 2] = 255
    img[0, :] = 0
    return img.astype(np.uint8)


def test_model_at_224(dev):
    """the full LDS footprint: two samples of four layers, with Equalize, Sharpness, a bicubic Rotate, both filters and a Contrast mean"""
    S = 224
    images = np.stack([_big(S, 1), _big(S, 2)])
    samples = [[R.layer(R.EQUALIZE), R.layer(R.SHARPNESS, factor=1.7), R.layer(R.ROTATE, R.BICUBIC, matrix=R.rotate_matrix(-23.5, S)),
                R.layer(R.CONTRAST, factor=0.4)],
               [R.layer(R.SHEAR_X, R.BILINEAR, matrix=R.affine_matrix(R.SHEAR_X, 0.27, S)), R.layer(R.AUTOCONTRAST), R.layer(R.COLOR, factor=1.9),
                R.layer(R.TRANSLATE_Y, R.BICUBIC, matrix=R.affine_matrix(R.TRANSLATE_Y, -0.31 * S, S))]]
    got = run_ops(dev, images, samples)
    for b in range(2):
        want = R.apply_layers(images[b], samples[b])
        assert chk(int((got[b] != want).sum()), 1), b
        assert (want != images[b]).mean() > 0.5


def test_model_at_32(dev, gold):
    images = gold["src32"][:5]
    samples = [[R.layer(R.ROTATE, R.BICUBIC, matrix=R.rotate_matrix(30.0, 32)), R.layer(R.SHARPNESS, factor=0.1)],
               [], [R.layer(R.SOLARIZE_ADD, arg=110), R.layer(R.EQUALIZE), R.layer(R.POSTERIZE, arg=1), R.layer(R.BRIGHTNESS, factor=1.9)],
               [R.layer(R.SHEAR_Y, R.BILINEAR, matrix=R.affine_matrix(R.SHEAR_Y, -0.3, 32))], [R.layer(R.AUTOCONTRAST), R.layer(R.INVERT)]]
    got = run_ops(dev, images, samples)
    for b in range(5):
        assert chk(int((got[b] != R.apply_layers(images[b], samples[b])).sum()), 1), b
    assert np.array_equal(got[1], images[1])


# ============================================================================================ the full stage
def to_table(rows):
    from devit_amd import data
    tab = np.zeros(len(rows), dtype=data.AUG_SAMPLE_DTYPE)
    for t, r in zip(tab, rows):
        for k in ("y0", "x0", "h", "w", "Rh", "Rw", "oy", "ox", "filter", "flip", "erase_mode", "noise_base"):
            t[k] = r[k]
        t["n_erase"] = len(r["erase"])
        for e, box in enumerate(r["erase"]):
            t["erase"][e] = box
    return tab


def run_batch(dev, src, idx, rows, S, seed, samples=None, spare_rows=2):
    """devit_augment_batch (samples None) or devit_augment_batch_ops into a sentinel-filled buffer -> fp32 [B,3,S,S] on the host"""
    from devit_amd import data
    B, n = len(rows), 3 * S * S
    flat = torch.full((GUARD + (B + spare_rows) * n + GUARD,), SENTINEL, dtype=torch.float32, device=dev)
    out = flat[GUARD:GUARD + (B + spare_rows) * n].view(B + spare_rows, 3, S, S)
    data.augment_batch(src, torch.tensor(idx, dtype=torch.int32, device=dev), to_table(rows), S, MEAN, STD, seed, out=out,
                       layers=None if samples is None else (samples if isinstance(samples, np.ndarray) else to_ops(samples)))
    got = flat.cpu().numpy()
    assert (got[:GUARD] == SENTINEL).all() and (got[GUARD + B * n:] == SENTINEL).all(), "wrote outside rows 0 .. B-1 of out"
    return got[GUARD:GUARD + B * n].reshape(B, 3, S, S)


def _rows(S, mode):
    boxes = [[(5, 7, 9, 13)], [(0, 0, 11, 6), (8, 3, 20, 30)], [(30, 30, 18, 18), (1, 40, 10, 7), (25, 35, 9, 9)],
             [(10, 10, 20, 20), (15, 15, 20, 20), (0, 44, 47, 4), (47, 0, 1, 47)], []]
    return [M.row(3 + b, 2, 20, 25 - b, S, filter=1 + b % 2, flip=b % 2, erase=e, erase_mode=mode, noise_base=(b << 33) + 5) for b, e in enumerate(boxes)]


@pytest.mark.parametrize("mode", [M.CONST, M.RAND, M.PIXEL])
def test_no_layers_is_the_plain_stage(dev, gold_aug, mode):
    """n_ops = 0 for every sample: the bits of devit_augment_batch, erasing included"""
    S, idx, seed = 48, [1, 3, 0, 2, 1], 0x9E3779B97F4A7C15
    src = torch.from_numpy(gold_aug["src32"]).to(dev)
    rows = _rows(S, mode)
    plain = run_batch(dev, src, idx, rows, S, seed)
    with_ops = run_batch(dev, src, idx, rows, S, seed, samples=[[] for _ in rows])
    assert np.array_equal(plain.view(np.uint32), with_ops.view(np.uint32))
    if mode == M.PIXEL:                                      # ... and at the padded crop of 32 and at 224
        for S2, r in ((32, M.row(-4, 3, 32, 32, 32, filter=0, flip=1, erase=[(20, 1, 12, 30)], erase_mode=mode, noise_base=3)),
                      (224, M.row(4, 6, 20, 17, 224, filter=1, flip=1, erase=[(190, 3, 34, 200)], erase_mode=mode, noise_base=2 ** 63))):
            a, b = run_batch(dev, src, [2], [r], S2, 77), run_batch(dev, src, [2], [r], S2, 77, samples=[[]])
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), S2


def test_full_path(dev, gold_aug):
    """crop and resize, flip, the layers, normalize, erase = tests/_augment_model.py with the op model between its flip and its normalize"""
    S, idx, seed = 48, [1, 3, 0, 2, 1], 99
    src = torch.from_numpy(gold_aug["src32"]).to(dev)
    rows = _rows(S, M.PIXEL)
    samples = [[R.layer(R.ROTATE, R.BICUBIC, matrix=R.rotate_matrix(17.0, S)), R.layer(R.COLOR, factor=1.6)], [R.layer(R.EQUALIZE)],
               [R.layer(R.SHARPNESS, factor=1.9), R.layer(R.SOLARIZE, arg=77), R.layer(R.TRANSLATE_X, R.BILINEAR, matrix=R.affine_matrix(R.TRANSLATE_X, 9.5, S)),
                R.layer(R.CONTRAST, factor=1.5)], [], [R.layer(R.BRIGHTNESS, factor=0.3), R.layer(R.AUTOCONTRAST)]]
    got = run_batch(dev, src, idx, rows, S, seed, samples=samples).astype(np.float64)
    for b, (i, r) in enumerate(zip(idx, rows)):
        u8 = M.resample(gold_aug["src32"][i], r, S)
        u8 = R.apply_layers(u8[:, ::-1] if r["flip"] else u8, samples[b])
        ref, bound = M.sample(gold_aug["src32"][i], dict(r, flip=0), S, MEAN, STD, seed, b, window=u8)
        err = np.abs(got[b] - ref)
        assert chk(float((err / np.maximum(bound, 1e-300)).max()), 1.0), b


# ============================================================================================ safety
def test_random_table_bytes_stay_inside(dev, gold_aug):
    """a table of random bytes (op ids, counts, filters, NaN and huge matrices, any fill) completes and writes nothing outside its rows"""
    from devit_amd import _lib, data, ops
    rng = np.random.RandomState(5)
    for S, B in ((32, 7), (224, 3)):
        raw = rng.randint(0, 256, B * data.AUG_OPS_DTYPE.itemsize).astype(np.uint8)
        tab = raw.view(data.AUG_OPS_DTYPE).copy()
        tab["n_ops"] = rng.randint(-3, 9, B)
        tab["op"][:, ::2] = rng.randint(-2, 17, (B, 2))      # half of the layers name real ops: the code behind them runs on the wild arguments
        tab["matrix"][0, 0] = (np.nan, 1e300, -np.inf, 1.0, 0.0, 3.0)
        imgs = torch.from_numpy(rng.randint(0, 256, (B, S, S, 3)).astype(np.uint8)).to(dev)
        n = B * S * S * 3
        flat = torch.full((GUARD + n + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
        ops.call("devit_image_ops", _lib.ptr(imgs), _lib.ptr(data.upload(tab.view(np.uint8).reshape(-1), dev)), B, S, _lib.ptr(flat[GUARD:]), _lib.stream_ptr())
        torch.cuda.synchronize()
        got = flat.cpu().numpy()
        assert (got[:GUARD] == 0xA5).all() and (got[GUARD + n:] == 0xA5).all()
    # the full stage with the same kind of table: sentinels around `out` (run_batch checks them); check_ops_table would refuse it, so it goes up raw
    src = torch.from_numpy(gold_aug["src32"]).to(dev)
    rows = _rows(48, M.RAND)
    tab = rng.randint(0, 256, 5 * data.AUG_OPS_DTYPE.itemsize).astype(np.uint8).view(data.AUG_OPS_DTYPE).copy()
    tab["op"][:, 1] = [3, 10, 1, 8, 14]
    B, n = 5, 3 * 48 * 48
    flat = torch.full((GUARD + (B + 1) * n + GUARD,), SENTINEL, dtype=torch.float32, device=dev)
    out = flat[GUARD:GUARD + (B + 1) * n].view(B + 1, 3, 48, 48)
    data.augment_batch(src, torch.tensor([0, 1, 2, 3, 0], dtype=torch.int32, device=dev), to_table(rows), 48, MEAN, STD, 1, out=out, layers=tab,
                       layers_dev=data.upload(tab.view(np.uint8).reshape(-1), dev))
    torch.cuda.synchronize()
    got = flat.cpu().numpy()
    assert (got[:GUARD] == SENTINEL).all() and (got[GUARD + B * n:] == SENTINEL).all() and (got[GUARD:GUARD + B * n] != SENTINEL).all()


# ============================================================================================ the loader and the CLI
def _layers_of(t):
    return [R.layer(int(t["op"][k]), int(t["filter"][k]), float(t["factor"][k]), int(t["arg"][k]), tuple(t["matrix"][k]), tuple(int(v) for v in t["fill"][k][:3]))
            for k in range(int(t["n_ops"]))]


@pytest.mark.parametrize("kw", [dict(auto_augment="rand-m9-mstd0.5-inc1", interpolation="random", re_prob=1.0, re_mode="pixel", re_count=2),
                                dict(color_jitter=0.4, interpolation="bilinear")])
def test_loader_batches_are_its_draws(dev, gold_aug, kw):
    from devit_amd import data
    imgs = np.concatenate([gold_aug["src32"]] * 2)
    ds = data.DeviceImageSet.from_arrays(imgs, np.arange(8), [str(i) for i in range(8)], device=dev)
    order = [5, 1, 1, 7, 0, 2, 6, 3]
    loader = data.DeviceLoader(ds, order, 4, data.TrainAugment(48, seed=21, rank=1, **kw), drop_last=True)
    twin = data.TrainAugment(48, seed=21, rank=1, **kw)
    applied = 0
    for k, (x, y) in enumerate(loader):
        idx = order[4 * k:4 * k + 4]
        tab, lay = twin.draw_with_ops(4, 32, 32)
        got = x.cpu().numpy().astype(np.float64)
        for b, (i, t) in enumerate(zip(idx, tab)):
            r = M.row(int(t["y0"]), int(t["x0"]), int(t["h"]), int(t["w"]), 48, filter=int(t["filter"]), flip=0,
                      erase=[tuple(int(v) for v in e) for e in t["erase"][:t["n_erase"]]], erase_mode=int(t["erase_mode"]), noise_base=int(t["noise_base"]))
            u8 = M.resample(imgs[i], r, 48)
            layers = _layers_of(lay[b])
            applied += len(layers)
            u8 = R.apply_layers(u8[:, ::-1] if t["flip"] else u8, layers)
            ref, bound = M.sample(imgs[i], r, 48, MEAN, STD, 21, b, window=u8)
            assert chk(float((np.abs(got[b] - ref) / np.maximum(bound, 1e-300)).max()), 1.0), (k, b)
        assert y.tolist() == idx
    assert applied >= 3


def test_distill_sub_cli_device_aug(dev, gold_aug, tmp_path):
    """distill_sub.py --device-data --device-aug with the default --aa and --color-jitter takes a step and evaluates"""
    Image = pytest.importorskip("PIL.Image")
    import devit_amd
    import distill_sub
    root = tmp_path / "data" / "sub-dataset0"
    for split, n in (("train_dataset", 260), ("test_dataset", 6)):
        for i in range(n):
            d = root / split / f"class{i % 5}"
            d.mkdir(parents=True, exist_ok=True)
            Image.fromarray(np.roll(gold_aug["src32"][i % 4], i, axis=1)).save(d / f"{i:04d}.png")
    tdir = tmp_path / "teacher" / "sub-dataset0"
    tdir.mkdir(parents=True)
    torch.manual_seed(0)
    torch.save(devit_amd.create_model("deit_base_distilled_patch16_224", num_classes=5, img_size=48).state_dict(), tdir / "checkpoint.pth")
    parser = argparse.ArgumentParser(parents=[distill_sub.get_args_parser()])
    args = parser.parse_args(["--device-data", "--device-aug", "--data-path", str(tmp_path / "data"), "--teacher-path", str(tmp_path / "teacher"),
                              "--batch-size", "64", "--eval-batch-size", "4", "--input-size", "48", "--epochs", "1", "--warmup-epochs", "0", "--model", "dedeit",
                              "--teacher-model", "deit_base_distilled_patch16_224", "--dataset", "cifar100", "--num_division", "20", "--reprob", "0.25",
                              "--train-interpolation", "random", "--output_dir", str(tmp_path / "out")])
    assert args.aa == "rand-m9-mstd0.5-inc1" and args.color_jitter == 0.4
    distill_sub.main(args)
    line = json.loads(open(os.path.join(args.output_dir, "sub-dataset0", "log.txt")).read().splitlines()[-1])
    assert np.isfinite(line["train_loss"]) and np.isfinite(line["test_loss"])
    ck = torch.load(os.path.join(args.output_dir, "sub-dataset0", "checkpoint_temp.pth"), map_location="cpu", weights_only=False)
    assert ck["data"]["drawn"] == 4 * 64
