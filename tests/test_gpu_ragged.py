"""The packed-set form of the input stage on the device (csrc/augment.hip: devit_augment_ragged; include/devit_hip.h, "Packed sets") against
tests/_ragged_model.py and PIL's own results (tests/golden/augment_ragged_pil.npz and augment_pil.npz; PIL is never imported for them): every
element within normalize_bound, about 2e-6 where neighbouring uint8 levels are >= 1.4e-2 apart, so passing proves the integer resampling exact,
through the narrow kernel, the wide one, and both for the same sample with identical bits.  Then clamping, a directory entry outside the arena,
erasing, the image-op layers, and devit_amd.data.DeviceLoader over a packed set end to end, distill_sub.py --device-data included."""
import argparse
import json
import os

import numpy as np
import pytest
import torch

import _augment_model as M
import _ragged_model as RM
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
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "augment_ragged_pil.npz")))


@pytest.fixture(scope="module")
def rset(dev, gold):
    """(the golden's sources as a packed set on the device, the images, the cases, the model's arena and directory)"""
    from devit_amd import data
    images, cases = RM.golden_set(gold)
    ds = data.DeviceImageSet.from_arrays(images, np.arange(len(images)) % 5, [str(i) for i in range(5)], device=dev, ragged=True)
    return ds, images, cases, *RM.pack(images)


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


def to_ops(samples):
    from devit_amd import data
    tab = np.zeros(len(samples), dtype=data.AUG_OPS_DTYPE)
    for t, layers in zip(tab, samples):
        t["n_ops"] = len(layers)
        for k, L in enumerate(layers):
            t["op"][k], t["filter"][k], t["factor"][k], t["arg"][k] = L["op"], L["filter"], L["factor"], L["arg"]
            t["matrix"][k] = L["matrix"]
            t["fill"][k][:3] = L["fill"]
    return tab


def run(dev, ds, idx, rows, S, seed=0, force_wide=False, samples=None, mean=MEAN, std=STD, spare_rows=2):
    """devit_augment_ragged into a sentinel-filled buffer with guards around it and `spare_rows` rows behind B -> fp32 [B,3,S,S] on the host,
    after checking that nothing but rows 0 .. B-1 was written"""
    from devit_amd import data
    B, n = len(rows), 3 * S * S
    flat = torch.full((GUARD + (B + spare_rows) * n + GUARD,), SENTINEL, dtype=torch.float32, device=dev)
    out = flat[GUARD:GUARD + (B + spare_rows) * n].view(B + spare_rows, 3, S, S)
    data.augment_ragged(ds, torch.tensor(idx, dtype=torch.int32, device=dev), to_table(rows), S, mean, std, seed, out=out, force_wide=force_wide,
                        layers=None if samples is None else to_ops(samples))
    got = flat.cpu().numpy()
    assert (got[:GUARD] == SENTINEL).all() and (got[GUARD + B * n:] == SENTINEL).all(), "wrote outside rows 0 .. B-1 of out"
    assert (got[GUARD:GUARD + B * n] != SENTINEL).all(), "a sample was left unwritten: neither kernel took it"
    return got[GUARD:GUARD + B * n].reshape(B, 3, S, S).astype(np.float64)


def worst(got, ref, bound):
    """max |got - ref| / bound (a zero bound asks for equality)"""
    err = np.abs(got - ref)
    return float(np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err > 0, np.inf, 0)).max())


def holds(got, u8):
    return chk(worst(got, M.normalize(u8, MEAN, STD), M.normalize_bound(u8, MEAN, STD)), 1.0)


# ============================================================================================ every golden case
def test_golden_cases(dev, rset):
    """batches of 1 .. 5 that mix sources, sizes and the two kernels; the cases' own indices repeat and come unordered; the flip on and off"""
    ds, images, cases, _, _ = rset
    total, sizes, mixed = 0, set(), 0
    for S in (48, 32, 224):
        group = [c for c in cases if c[2] == S]
        group = group[::2] + group[1::2]                    # the file lists a source's cases together: interleave them
        at, B = 0, 1
        while at < len(group):
            part = group[at:at + B]
            kinds = {RM.is_wide(r) for _, r, _, _ in part}
            mixed += len(kinds) == 2 and len({i for i, _, _, _ in part}) > 1
            for phase in (0, 1):
                rows = [dict(r, flip=(b + phase) % 2) for b, (_, r, _, _) in enumerate(part)]
                got = run(dev, ds, [i for i, _, _, _ in part], rows, S)
                wide = run(dev, ds, [i for i, _, _, _ in part], rows, S, force_wide=True) if S < 224 or phase == 0 else got
                assert np.array_equal(got, wide), (S, at)                 # every sample through the wide kernel: the same bits
                for b, ((_, _, _, px), r) in enumerate(zip(part, rows)):
                    assert holds(got[b], px[:, ::-1] if r["flip"] else px), (S, r)
            total += len(part)
            sizes.add(len(part))
            at, B = at + B, B % 5 + 1
    assert total == len(cases) and sizes >= {1, 2, 3, 4, 5} and mixed >= 3


def test_the_uniform_golden_packed(dev):
    """the 49 cases of augment_pil.npz as a packed set: once as the split decides (all narrow), once through the wide kernel; identical bits"""
    from devit_amd import data
    g = dict(np.load(os.path.join(ROOT, "tests", "golden", "augment_pil.npz")))
    images, first = [], {}
    for s, name in enumerate(g["sources"]):
        first[s] = len(images)
        images += list(g[str(name)])
    ds = data.DeviceImageSet.from_arrays(images, np.zeros(len(images), np.int64), ["0"], device=dev, ragged=True)
    cases = [(first[int(c[0])] + int(c[1]), r, S, px) for c, (_, r, S, px) in zip(g["cases"], M.golden_cases(g))]
    assert len(cases) == 49 and not any(RM.is_wide(r) for _, r, _, _ in cases)
    for S in sorted({c[2] for c in cases}):
        group = [c for c in cases if c[2] == S]
        for at in range(0, len(group), 7):
            part = group[at:at + 7]
            rows = [dict(r, flip=b % 2) for b, (_, r, _, _) in enumerate(part)]
            idx = [i for i, _, _, _ in part]
            got, wide = run(dev, ds, idx, rows, S), run(dev, ds, idx, rows, S, force_wide=True)
            assert np.array_equal(got, wide), (S, at)
            for b, ((_, _, _, px), r) in enumerate(zip(part, rows)):
                assert holds(got[b], px[:, ::-1] if r["flip"] else px) and holds(wide[b], px[:, ::-1] if r["flip"] else px), (S, r)


def test_unordered_repeated_indices_and_clamping(dev, rset):
    """an index outside the set is clamped, not followed: the table row then meets the clamped image"""
    ds, images, _, arena, entries = rset
    n = len(images)
    r_first, r_last = M.row(2, 3, 100, 90, 48), M.row(1, 20, 50, 200, 48, filter=M.BILINEAR)      # image 0 is 146 x 145, the last one 61 x 330
    idx, rows = [n - 1, 0, n - 1, 0, 99, -5], [r_last, r_first, r_last, r_first, r_last, r_first]
    got = run(dev, ds, idx, rows, 48)
    for b, (i, r) in enumerate(zip([n - 1, 0, n - 1, 0, n - 1, 0], rows)):
        assert holds(got[b], RM.window(arena, entries, i, r, 48)), b
    assert np.array_equal(got[0], got[2]) and np.array_equal(got[0], got[4]) and np.array_equal(got[1], got[5])


def test_an_entry_past_the_arena_gives_zeros(dev, rset):
    """a directory the host would have refused, handed to the C entry directly: the sample whose entry reaches past the arena (or has no extent)
    reads as an image of zeros, its neighbours are served, nothing outside `out` is written; through both kernels"""
    from devit_amd import _lib, data, ops
    ds, images, _, arena, entries = rset
    ent = ds.entries.cpu().numpy().view(data.IMAGE_ENTRY_DTYPE).copy()
    sizes = [images[i].shape[:2] for i in range(4)]
    ent["offset"][1] = arena.size - 64                       # a 150 x 170 image 64 bytes before the end
    ent["H"][2], ent["offset"][3] = -7, 2 ** 63
    ent_dev = torch.from_numpy(ent.view(np.uint8).reshape(-1).copy()).to(dev)
    S, B = 48, 4
    rows = [M.row(0, 0, h, w, S) for h, w in sizes]
    tab = data.upload(to_table(rows).view(np.uint8).reshape(-1), dev)
    idx = torch.tensor([0, 1, 2, 3], dtype=torch.int32, device=dev)
    T = RM.max_taps(rows)
    nbytes = _lib.load().devit_augment_ragged_workspace(B, S, T, 0)
    assert nbytes == B * 2 * (2 + T) * S * 4
    m3, s3 = (_lib.C.c_float * 3)(*MEAN), (_lib.C.c_float * 3)(*STD)
    zeros = np.zeros((S, S, 3), np.uint8)
    for flags in (0, _lib.AUGMENT_FORCE_WIDE):
        flat = torch.full((GUARD + (B + 1) * 3 * S * S + GUARD,), SENTINEL, dtype=torch.float32, device=dev)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        ops.call("devit_augment_ragged", _lib.ptr(ds.arena), ds.arena.shape[0], _lib.ptr(ent_dev), len(ds), _lib.ptr(idx), _lib.ptr(tab), None, B, S, m3, s3, 0,
                 _lib.ptr(flat[GUARD:]), _lib.ptr(ws), nbytes, T, flags, _lib.stream_ptr())
        torch.cuda.synchronize()
        got = flat.cpu().numpy()
        assert (got[:GUARD] == SENTINEL).all() and (got[GUARD + B * 3 * S * S:] == SENTINEL).all()
        got = got[GUARD:GUARD + B * 3 * S * S].reshape(B, 3, S, S).astype(np.float64)
        assert holds(got[0], RM.window(arena, entries, 0, rows[0], S))
        for b in (1, 2, 3):
            assert holds(got[b], zeros), (flags, b)


# ============================================================================================ erasing
ERASE_SEED = 0x9E3779B97F4A7C15


@pytest.mark.parametrize("mode", [M.CONST, M.RAND, M.PIXEL])
def test_erasing_on_a_mixed_batch(dev, rset, mode):
    ds, images, _, arena, entries = rset
    S = 48
    boxes = [[(5, 7, 9, 13)], [(0, 0, 11, 6), (8, 3, 20, 30)], [(30, 30, 18, 18), (1, 40, 10, 7), (25, 35, 9, 9)],
             [(10, 10, 20, 20), (15, 15, 20, 20), (0, 44, 47, 4), (47, 0, 1, 47)], []]
    idx = [5, 0, 2, 6, 3]
    rows = []
    for b, (i, e) in enumerate(zip(idx, boxes)):
        H, W = images[i].shape[:2]
        rows.append(M.row(b, 1, H - 2 * b, W - 3, S, filter=1 + b % 2, flip=b % 2, erase=e, erase_mode=mode, noise_base=(b << 33) + 5))
    assert {RM.is_wide(r) for r in rows} == {True, False}
    got = run(dev, ds, idx, rows, S, ERASE_SEED)
    ref, bound = RM.batch(arena, entries, idx, rows, S, MEAN, STD, ERASE_SEED)
    assert chk(worst(got, ref, bound), 1.0)
    assert np.array_equal(got, run(dev, ds, idx, rows, S, ERASE_SEED, force_wide=True))
    plain = run(dev, ds, idx, [dict(r, erase=[]) for r in rows], S, ERASE_SEED)
    for b, r in enumerate(rows):
        inside = np.zeros((S, S), bool)
        for m in M.erase_masks(r, S):
            inside |= m
        assert np.array_equal(got[b][:, ~inside], plain[b][:, ~inside]), b
        if r["erase"]:
            assert (got[b][:, inside] != plain[b][:, inside]).mean() > 0.99


def test_erasing_at_224_through_the_wide_kernel(dev, rset):
    ds, images, _, arena, entries = rset
    i = next(k for k, im in enumerate(images) if im.shape[:2] == (40, 700))
    r = M.row(0, 0, 40, 700, 224, flip=1, erase=[(190, 3, 34, 200), (0, 220, 100, 4)], erase_mode=M.PIXEL, noise_base=2 ** 63)
    got = run(dev, ds, [i], [r], 224, 77)
    ref, bound = RM.batch(arena, entries, [i], [r], 224, MEAN, STD, 77)
    assert RM.is_wide(r) and chk(worst(got, ref, bound), 1.0)


# ============================================================================================ the image-op layers
def _op_case(images, S):
    idx = [3, 0, 5, 6, 1]
    rows = [M.row(0, 0, *images[i].shape[:2], S, filter=1 + b % 2, flip=b % 2) for b, i in enumerate(idx)]
    samples = [[R.layer(R.ROTATE, R.BICUBIC, matrix=R.rotate_matrix(17.0, S)), R.layer(R.COLOR, factor=1.6)], [R.layer(R.EQUALIZE)],
               [R.layer(R.SHARPNESS, factor=1.9), R.layer(R.SOLARIZE, arg=77), R.layer(R.TRANSLATE_X, R.BILINEAR, matrix=R.affine_matrix(R.TRANSLATE_X, 9.5, S)),
                R.layer(R.CONTRAST, factor=1.5)], [], [R.layer(R.BRIGHTNESS, factor=0.3), R.layer(R.AUTOCONTRAST)]]
    return idx, rows, samples


def test_ops_window_byte_for_byte(dev, rset):
    """with mean 0 and std 1 the output is level / 255 in fp32, which names the level: the uint8 window after the layers, byte for byte"""
    ds, images, _, arena, entries = rset
    S = 48
    idx, rows, samples = _op_case(images, S)
    assert {RM.is_wide(r) for r in rows} == {True, False}
    got = run(dev, ds, idx, rows, S, samples=samples, mean=(0., 0., 0.), std=(1., 1., 1.))
    levels = np.rint(got * 255.0)
    assert np.abs(got * 255.0 - levels).max() < 1e-4
    for b, (i, r) in enumerate(zip(idx, rows)):
        u8 = RM.window(arena, entries, i, r, S)
        want = R.apply_layers(u8[:, ::-1] if r["flip"] else u8, samples[b])
        assert chk(int((np.moveaxis(levels[b], 0, 2) != want).sum()), 1), b
    none = run(dev, ds, idx, rows, S, samples=[[]] * 5)          # no layers: the bits of the call without a layer table
    assert np.array_equal(none, run(dev, ds, idx, rows, S))


def test_ops_full_stage(dev, rset):
    ds, images, _, arena, entries = rset
    S, seed = 48, 99
    idx, rows, samples = _op_case(images, S)
    rows = [dict(r, erase=[(4 + b, 3, 10, 20 + b)], erase_mode=M.PIXEL, noise_base=7 + (b << 20)) for b, r in enumerate(rows)]
    got = run(dev, ds, idx, rows, S, seed, samples=samples)
    assert np.array_equal(got, run(dev, ds, idx, rows, S, seed, samples=samples, force_wide=True))
    for b, (i, r) in enumerate(zip(idx, rows)):
        u8 = RM.window(arena, entries, i, r, S)
        u8 = R.apply_layers(u8[:, ::-1] if r["flip"] else u8, samples[b])
        ref, bound = M.sample(None, dict(r, flip=0), S, MEAN, STD, seed, b, window=u8)
        assert chk(float((np.abs(got[b] - ref) / np.maximum(bound, 1e-300)).max()), 1.0), b


# ============================================================================================ the loader, end to end
def test_loader_eval_and_train_streams(dev, rset):
    """the loaders' batches are their transforms' draws on each image's own size through the stage: regenerated from twin transforms"""
    from devit_amd import data
    ds, images, _, arena, entries = rset
    n = len(images)
    ev = data.DeviceLoader(ds, torch.utils.data.SequentialSampler(ds), 4, data.EvalTransform(48), drop_last=False)
    batches = list(ev)
    assert len(ev) == 2 and [tuple(x.shape) for x, _ in batches] == [(4, 3, 48, 48), (n - 4, 3, 48, 48)]
    assert torch.cat([y for _, y in batches]).tolist() == [i % 5 for i in range(n)]
    got = torch.cat([x for x, _ in batches]).cpu().numpy().astype(np.float64)
    for i in range(n):
        H, W = images[i].shape[:2]
        r = M.row(0, 0, H, W, 48, *RM.eval_geometry(H, W, 48))
        assert holds(got[i], RM.window(arena, entries, i, r, 48)), i
    kw = dict(interpolation='random', re_prob=1.0, re_mode='pixel', re_count=3, seed=21, rank=1)
    order = [5, 1, 1, 6, 0, 2, 3]
    loader = data.DeviceLoader(ds, order, 3, data.TrainAugment(48, **kw), drop_last=True)
    twin = data.TrainAugment(48, **kw)
    for k, (x, y) in enumerate(loader):
        idx = order[3 * k:3 * k + 3]
        tab = twin.draw(3, ds.sizes[idx, 0], ds.sizes[idx, 1])
        rows = [M.row(int(t["y0"]), int(t["x0"]), int(t["h"]), int(t["w"]), 48, filter=int(t["filter"]), flip=int(t["flip"]),
                      erase=[tuple(int(v) for v in e) for e in t["erase"][:t["n_erase"]]], erase_mode=int(t["erase_mode"]), noise_base=int(t["noise_base"])) for t in tab]
        ref, bound = RM.batch(arena, entries, idx, rows, 48, MEAN, STD, 21)
        assert chk(worst(x.cpu().numpy().astype(np.float64), ref, bound), 1.0), k
        assert y.tolist() == [i % 5 for i in idx]


def test_step_and_evaluate_from_a_packed_set(dev, rset):
    """one distillation step (Mixup on: bf16 patch rows) and one evaluate straight from DeviceLoaders over a packed set; then the f32 path"""
    import devit_amd
    import distill_sub
    from devit_amd import data, engine, ops
    ds = rset[0]
    torch.manual_seed(3)
    student = devit_amd.create_model("dedeit", depth=2, num_classes=5, img_size=48).to(dev).train()
    teacher = devit_amd.create_model("deit_base_distilled_patch16_224", depth=2, num_classes=5, img_size=48).to(dev).eval()
    train = data.DeviceLoader(ds, [0, 1, 2, 3, 4, 5, 6, 0], 4, data.TrainAugment(48, re_prob=0.5, re_mode='pixel', seed=1), drop_last=True)
    val = data.DeviceLoader(ds, torch.utils.data.SequentialSampler(ds), 8, data.EvalTransform(48), drop_last=False)
    mix = distill_sub.Mixup(0.8, 1.0, 1.0, 0.5, 0.1, 5, mode="elem", img_size=48)
    mix.set_precisions(student.precision, teacher.precision)
    np.random.seed(2)
    batches = engine._PreparedBatches(train, dev, mix, None)
    samples, targets, _ = next(iter(batches))
    assert isinstance(samples, ops.PatchRows) and tuple(targets.shape) == (4, 5)
    out = engine.distill_forward(student, teacher, samples, targets)
    out["loss"].backward()
    g = student.blocks[1].mlp.fc1.weight.grad
    assert np.isfinite(float(out["loss"])) and g is not None and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0
    stats = engine.evaluate(val, student, dev)
    assert np.isfinite(stats["loss"]) and 0 <= stats["acc1"] <= 100
    student.precision = "f32"
    mix.set_precisions("f32")
    x, y = next(iter(train))
    mixed, t = mix(x, y)
    assert torch.is_tensor(mixed) and mixed.dtype == torch.float32 and tuple(mixed.shape) == (4, 3, 48, 48)
    student.eval()
    with torch.no_grad():
        logits = student(mixed)
    assert bool(torch.isfinite(logits).all())


@pytest.mark.parametrize("aug", [False, True])
def test_distill_sub_cli_on_a_mixed_division_tree(dev, gold, tmp_path, aug):
    Image = pytest.importorskip("PIL.Image")
    import devit_amd
    import distill_sub
    images = RM.golden_set(gold)[0]
    root = tmp_path / "data" / "sub-dataset0"
    for split, n in (("train_dataset", 260), ("test_dataset", 7)):
        for i in range(n):
            d = root / split / f"class{i % 5}"
            d.mkdir(parents=True, exist_ok=True)
            Image.fromarray(np.roll(images[i % 7], i, axis=1)).save(d / f"{i:04d}.png")
    tdir = tmp_path / "teacher" / "sub-dataset0"
    tdir.mkdir(parents=True)
    torch.manual_seed(0)
    torch.save(devit_amd.create_model("deit_base_distilled_patch16_224", num_classes=5, img_size=48).state_dict(), tdir / "checkpoint.pth")
    parser = argparse.ArgumentParser(parents=[distill_sub.get_args_parser()])
    args = parser.parse_args(["--device-data"] + (["--device-aug"] if aug else ["--aa", "none", "--color-jitter", "0"]) +
                             ["--data-path", str(tmp_path / "data"), "--teacher-path", str(tmp_path / "teacher"), "--device-data-cache", str(tmp_path / "cache"),
                              "--batch-size", "64", "--eval-batch-size", "4", "--input-size", "48", "--epochs", "1", "--warmup-epochs", "0", "--model", "dedeit",
                              "--teacher-model", "deit_base_distilled_patch16_224", "--dataset", "cifar100", "--num_division", "20", "--reprob", "0.5",
                              "--recount", "2", "--train-interpolation", "random", "--output_dir", str(tmp_path / "out")])
    distill_sub.main(args)
    line = json.loads(open(os.path.join(args.output_dir, "sub-dataset0", "log.txt")).read().splitlines()[-1])
    assert np.isfinite(line["train_loss"]) and np.isfinite(line["test_loss"])
    ck = torch.load(os.path.join(args.output_dir, "sub-dataset0", "checkpoint_temp.pth"), map_location="cpu", weights_only=False)
    assert ck["data"]["drawn"] == 4 * 64
    assert os.path.exists(tmp_path / "cache" / "train" / "arena.npy") and os.path.exists(tmp_path / "cache" / "test" / "arena.npy")
