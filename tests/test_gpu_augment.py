"""The input-augmentation stage on the device (csrc/augment.hip: devit_augment_batch) against tests/_augment_model.py and PIL's own results
(tests/golden/augment_pil.npz; PIL is never imported here): every element within the bounds the model file derives from the roundings
involved.  Neighbouring uint8 levels are >= 1.4e-2 apart after the normalization and the bound is about 2e-6, so passing proves the integer
resampling exact.  Then erasing against the Philox definition, and devit_amd.data.DeviceLoader end to end at 48 pixels: against the golden,
through one distillation step and one evaluate with Mixup on (bf16 patch rows and the f32 path), and through distill_sub.py --device-data."""
import argparse
import json
import os

import numpy as np
import pytest
import torch

import _augment_model as M
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
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "augment_pil.npz")))


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


def run(dev, src, idx, rows, S, seed=0, spare_rows=2):
    """devit_augment_batch into a sentinel-filled buffer with guards around it and `spare_rows` rows behind B -> fp32 [B,3,S,S] on the host,
    after checking that nothing but rows 0 .. B-1 was written"""
    from devit_amd import data
    B, n = len(rows), 3 * S * S
    flat = torch.full((GUARD + (B + spare_rows) * n + GUARD,), SENTINEL, dtype=torch.float32, device=dev)
    out = flat[GUARD:GUARD + (B + spare_rows) * n].view(B + spare_rows, 3, S, S)
    data.augment_batch(src, torch.tensor(idx, dtype=torch.int32, device=dev), to_table(rows), S, MEAN, STD, seed, out=out)
    got = flat.cpu().numpy()
    assert (got[:GUARD] == SENTINEL).all() and (got[GUARD + B * n:] == SENTINEL).all(), "wrote outside rows 0 .. B-1 of out"
    return got[GUARD:GUARD + B * n].reshape(B, 3, S, S).astype(np.float64)


def worst(got, ref, bound):
    """max |got - ref| / bound (a zero bound asks for equality)"""
    err = np.abs(got - ref)
    return float(np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err > 0, np.inf, 0)).max())


# ============================================================================================ every golden case
def test_golden_cases(dev, gold):
    cases = M.golden_cases(gold)
    groups = {}
    for c, (img, r, S, px) in zip(gold["cases"], cases):
        groups.setdefault((int(c[0]), S), []).append((int(c[1]), r, px))
    total, sizes = 0, set()
    for (s, S), group in sorted(groups.items()):
        src = torch.from_numpy(gold[str(gold["sources"][s])]).to(dev)
        at, B = 0, 1
        while at < len(group):                              # batches of 1, 2, .. 5, 1, ..: the cases' own indices repeat and come unordered
            part = group[at:at + B]
            for phase in (0, 1):                            # every case with the flip on and off
                rows = [dict(r, flip=(b + phase) % 2) for b, (_, r, _) in enumerate(part)]
                got = run(dev, src, [i for i, _, _ in part], rows, S)
                for b, ((_, _, px), r) in enumerate(zip(part, rows)):
                    u8 = px[:, ::-1] if r["flip"] else px
                    assert chk(worst(got[b], M.normalize(u8, MEAN, STD), M.normalize_bound(u8, MEAN, STD)), 1.0), (s, S, r)
            total += len(part)
            sizes.add(len(part))
            at, B = at + B, B % 5 + 1
    assert total == len(cases) and sizes >= {1, 2, 3, 4, 5}


def test_unordered_repeated_indices_and_clamping(dev, gold):
    """idx need not be sorted or distinct, and an index outside the set is clamped, not followed"""
    src = torch.from_numpy(gold["src32"]).to(dev)
    S, r = 48, M.row(2, 3, 25, 20, 48, filter=M.BICUBIC)
    got = run(dev, src, [3, 0, 3, 1, 0, 99, -5], [r] * 7, S)
    for b, i in enumerate([3, 0, 3, 1, 0, 3, 0]):
        u8 = M.resample(gold["src32"][i], r, S)
        assert chk(worst(got[b], M.normalize(u8, MEAN, STD), M.normalize_bound(u8, MEAN, STD)), 1.0), b
    assert np.array_equal(got[0], got[2]) and np.array_equal(got[1], got[4])


# ============================================================================================ erasing
ERASE_SEED = 0x9E3779B97F4A7C15


def erase_rows(S, mode):
    """1 to 4 boxes, overlapping ones included, a box at each border, on crops with and without the flip"""
    boxes = [[(5, 7, 9, 13)], [(0, 0, 11, 6), (8, 3, 20, 30)], [(30, 30, 18, 18), (1, 40, 10, 7), (25, 35, 9, 9)],
             [(10, 10, 20, 20), (15, 15, 20, 20), (0, 44, 47, 4), (47, 0, 1, 47)], []]
    return [M.row(3 + b, 2, 20, 25 - b, S, filter=1 + b % 2, flip=b % 2, erase=e, erase_mode=mode, noise_base=(b << 33) + 5) for b, e in enumerate(boxes)]


@pytest.mark.parametrize("mode", [M.CONST, M.RAND, M.PIXEL])
def test_erasing(dev, gold, mode):
    S, idx = 48, [1, 3, 0, 2, 1]
    src = torch.from_numpy(gold["src32"]).to(dev)
    rows = erase_rows(S, mode)
    got = run(dev, src, idx, rows, S, ERASE_SEED)
    ref, bound = M.batch(gold["src32"], idx, rows, S, MEAN, STD, ERASE_SEED)
    assert chk(worst(got, ref, bound), 1.0)
    plain = run(dev, src, idx, [dict(r, erase=[]) for r in rows], S, ERASE_SEED)
    for b, r in enumerate(rows):
        inside = np.zeros((S, S), bool)
        for m in M.erase_masks(r, S):
            inside |= m
        assert np.array_equal(got[b][:, ~inside], plain[b][:, ~inside]), b               # outside the boxes: the bits of the run without erasing
        if r["erase"]:
            assert inside.any() and (got[b][:, inside] != plain[b][:, inside]).mean() > 0.99
    assert np.array_equal(got, run(dev, src, idx, rows, S, ERASE_SEED))                  # same seed: same bits
    if mode != M.CONST:
        for other in (run(dev, src, idx, rows, S, ERASE_SEED + 1), run(dev, src, idx, [dict(r, noise_base=r["noise_base"] + 1) for r in rows], S, ERASE_SEED)):
            for b, r in enumerate(rows[:4]):
                inside = M.erase_masks(r, S)[-1]
                assert (other[b][:, inside] != got[b][:, inside]).mean() > 0.99, b       # another seed / another counter base: other noise
                assert np.array_equal(other[b][:, ~inside & ~np.any(M.erase_masks(r, S), axis=0)], got[b][:, ~inside & ~np.any(M.erase_masks(r, S), axis=0)])
    if mode == M.PIXEL:                                          # the counter is noise_base + b: samples 0 and 1 share N = 11, sample 2 has N = 13
        rows3 = [M.row(0, 0, 32, 32, S, erase=[(0, 0, 40, 40)], erase_mode=mode, noise_base=nb) for nb in (11, 10, 11)]
        a = run(dev, src, [0, 0, 0], rows3, S, ERASE_SEED)
        assert np.array_equal(a[0], a[1]) and (a[2][:, :40, :40] != a[0][:, :40, :40]).mean() > 0.99


def test_erasing_at_224_and_32(dev, gold):
    """the pixel-noise counters at the largest and smallest sides (pixel groups up to 12543; several bands), on the padded crop too"""
    src = torch.from_numpy(gold["src32"]).to(dev)
    for S, r in ((224, M.row(4, 6, 20, 17, 224, filter=1, flip=1, erase=[(190, 3, 34, 200), (0, 220, 100, 4)], erase_mode=M.PIXEL, noise_base=2 ** 63)),
                 (32, M.row(-4, 3, 32, 32, 32, filter=0, flip=1, erase=[(20, 1, 12, 30)], erase_mode=M.RAND, noise_base=3))):
        got = run(dev, src, [2], [r], S, 77)
        ref, bound = M.batch(gold["src32"], [2], [r], S, MEAN, STD, 77)
        assert chk(worst(got, ref, bound), 1.0), S


# ============================================================================================ the loader, end to end
def _set(dev, gold, n=8, classes=10):
    from devit_amd import data
    imgs = np.concatenate([gold["src32"]] * ((n + 3) // 4))[:n]
    return data.DeviceImageSet.from_arrays(imgs, np.arange(n) % classes, [str(i) for i in range(classes)], device=dev)


def test_loader_eval_equals_the_golden_path(dev, gold):
    from devit_amd import data
    ds = _set(dev, gold, 6)
    loader = data.DeviceLoader(ds, torch.utils.data.SequentialSampler(ds), 4, data.EvalTransform(48), drop_last=False)
    batches = list(loader)
    assert len(loader) == 2 and [tuple(x.shape) for x, _ in batches] == [(4, 3, 48, 48), (2, 3, 48, 48)]
    assert torch.cat([y for _, y in batches]).tolist() == [0, 1, 2, 3, 4, 5] and batches[0][1].dtype == torch.int64
    assert batches[0][0].data_ptr() != batches[1][0].data_ptr() and batches[0][0].dtype == torch.float32
    got = torch.cat([x for x, _ in batches]).cpu().numpy().astype(np.float64)
    case = [(r, px) for (img, r, S, px), c in zip(M.golden_cases(gold), gold["cases"]) if S == 48 and r["Rh"] == 54 and r["Rw"] == 54 and int(c[1]) == 2]
    assert len(case) == 1
    r, px = case[0]
    assert chk(worst(got[2], M.normalize(px, MEAN, STD), M.normalize_bound(px, MEAN, STD)), 1.0)        # PIL's own eval-geometry result
    for b in range(6):
        u8 = M.resample(gold["src32"][b % 4], r, 48)
        assert chk(worst(got[b], M.normalize(u8, MEAN, STD), M.normalize_bound(u8, MEAN, STD)), 1.0), b


def test_loader_train_stream(dev, gold):
    """the train loader's batches are its transform's draws through the stage: regenerated from a twin transform, erasing included"""
    from devit_amd import data
    ds = _set(dev, gold, 8)
    kw = dict(interpolation='random', re_prob=1.0, re_mode='pixel', re_count=3, seed=21, rank=1)
    order = [5, 1, 1, 7, 0, 2, 6]
    loader = data.DeviceLoader(ds, order, 3, data.TrainAugment(48, **kw), drop_last=True)
    twin = data.TrainAugment(48, **kw)
    assert len(loader) == 2
    for k, (x, y) in enumerate(loader):
        idx = order[3 * k:3 * k + 3]
        tab = twin.draw(3, 32, 32)
        rows = [M.row(int(t["y0"]), int(t["x0"]), int(t["h"]), int(t["w"]), 48, filter=int(t["filter"]), flip=int(t["flip"]),
                      erase=[tuple(int(v) for v in e) for e in t["erase"][:t["n_erase"]]], erase_mode=int(t["erase_mode"]), noise_base=int(t["noise_base"])) for t in tab]
        ref, bound = M.batch(gold["src32"], [i % 4 for i in idx], rows, 48, MEAN, STD, 21)
        assert chk(worst(x.cpu().numpy().astype(np.float64), ref, bound), 1.0), k
        assert y.tolist() == idx


def test_step_and_evaluate_from_the_loader(dev, gold):
    """one distillation step (Mixup on: bf16 patch rows) and one evaluate run straight from DeviceLoaders; then the f32 path"""
    import devit_amd
    import distill_sub
    from devit_amd import data, engine, ops
    ds = _set(dev, gold, 8)
    torch.manual_seed(3)
    student = devit_amd.create_model("dedeit", depth=2, num_classes=10, img_size=48).to(dev).train()
    teacher = devit_amd.create_model("deit_base_distilled_patch16_224", depth=2, num_classes=10, img_size=48).to(dev).eval()
    train = data.DeviceLoader(ds, list(range(8)), 4, data.TrainAugment(48, re_prob=0.5, re_mode='pixel', seed=1), drop_last=True)
    val = data.DeviceLoader(ds, torch.utils.data.SequentialSampler(ds), 8, data.EvalTransform(48), drop_last=False)
    mix = distill_sub.Mixup(0.8, 1.0, 1.0, 0.5, 0.1, 10, mode="elem", img_size=48)
    mix.set_precisions(student.precision, teacher.precision)
    np.random.seed(2)
    batches = engine._PreparedBatches(train, dev, mix, None)
    samples, targets, _ = next(iter(batches))
    assert isinstance(samples, ops.PatchRows) and tuple(targets.shape) == (4, 10)
    out = engine.distill_forward(student, teacher, samples, targets)
    out["loss"].backward()
    g = student.blocks[1].mlp.fc1.weight.grad
    assert np.isfinite(float(out["loss"])) and g is not None and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0
    stats = engine.evaluate(val, student, dev)
    assert np.isfinite(stats["loss"]) and 0 <= stats["acc1"] <= 100
    student.precision = "f32"                               # an "f32" reader: the mixed batch stays an fp32 image tensor
    mix.set_precisions("f32")
    x, y = next(iter(train))
    mixed, t = mix(x, y)
    assert torch.is_tensor(mixed) and mixed.dtype == torch.float32 and tuple(mixed.shape) == (4, 3, 48, 48)
    student.eval()
    with torch.no_grad():
        logits = student(mixed)
    assert bool(torch.isfinite(logits).all())


def test_distill_sub_cli_device_data(dev, gold, tmp_path):
    Image = pytest.importorskip("PIL.Image")
    import devit_amd
    import distill_sub
    root = tmp_path / "data" / "sub-dataset0"
    for split, n in (("train_dataset", 260), ("test_dataset", 6)):
        for i in range(n):
            d = root / split / f"class{i % 5}"
            d.mkdir(parents=True, exist_ok=True)
            Image.fromarray(np.roll(gold["src32"][i % 4], i, axis=1)).save(d / f"{i:04d}.png")
    tdir = tmp_path / "teacher" / "sub-dataset0"
    tdir.mkdir(parents=True)
    torch.manual_seed(0)
    torch.save(devit_amd.create_model("deit_base_distilled_patch16_224", num_classes=5, img_size=48).state_dict(), tdir / "checkpoint.pth")
    parser = argparse.ArgumentParser(parents=[distill_sub.get_args_parser()])
    args = parser.parse_args(["--device-data", "--aa", "none", "--color-jitter", "0", "--data-path", str(tmp_path / "data"), "--teacher-path", str(tmp_path / "teacher"),
                              "--batch-size", "64", "--eval-batch-size", "4", "--input-size", "48", "--epochs", "1", "--warmup-epochs", "0", "--model", "dedeit",
                              "--teacher-model", "deit_base_distilled_patch16_224", "--dataset", "cifar100", "--num_division", "20", "--reprob", "0.5",
                              "--recount", "2", "--train-interpolation", "random", "--output_dir", str(tmp_path / "out")])
    distill_sub.main(args)
    line = json.loads(open(os.path.join(args.output_dir, "sub-dataset0", "log.txt")).read().splitlines()[-1])
    assert np.isfinite(line["train_loss"]) and np.isfinite(line["test_loss"])
    ck = torch.load(os.path.join(args.output_dir, "sub-dataset0", "checkpoint_temp.pth"), map_location="cpu", weights_only=False)
    assert ck["data"]["drawn"] == 4 * 64                    # 256 draws of the repeated-augmentation epoch, in whole batches: the stream's state travels
