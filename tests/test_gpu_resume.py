"""--resume under --deterministic at world size 1: stopping after an epoch and resuming gives the bits of the run that was never stopped.

Every case runs distill_sub.main three times in this process: A (three epochs of three steps), A' (the same again: the control -- without it
the comparison below means nothing) and B (a fresh main() resumed from A's epoch-0 checkpoint into another directory).  B's checkpoints after
epochs 1 and 2 and its log lines must equal A's: weights, EMA, optimizer moments, step count, learning rate, schedule, the loader's draw stream.
No tolerance and no reference numbers: the uninterrupted run is the reference.  The epoch checkpoints are collected by wrapping
utils.save_on_master for the duration of a run (checkpoint_temp.pth is overwritten every epoch)."""
import argparse
import ast
import hashlib
import json
import os
import shutil

import numpy as np
import pytest
import torch

from devit_amd import optim

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def common(synthetic=3, size=64, batch=4, division=4, epochs=3):
    """the flags every run here shares: three epochs of three steps at 64 pixels (18 tokens), batch 4"""
    return ["--deterministic", "--batch-size", str(batch), "--epochs", str(epochs), "--warmup-epochs", "0", "--model", "dedeit",
            "--teacher-model", "deit_base_distilled_patch16_224", "--dataset", "cifar100", "--num_division", str(division), "--model-ema",
            "--input-size", str(size)] + (["--synthetic", str(synthetic)] if synthetic else [])


COMMON = common()


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from devit_amd import _lib
    _lib.require_device(torch.zeros(1, device="cuda"))
    return torch.device("cuda")


# ---- the comparison ---------------------------------------------------------------------------------------------------------------------------

def bits(x):
    """the tensor's bits as integers (tests/test_gpu_relfused.py): NaNs and signed zeros compare as what they are"""
    return x.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[x.element_size()])


def _diff(a, b, path):
    """None, or what differs first below `path`: tensors by their bits, containers entry by entry, everything else by =="""
    if isinstance(a, torch.Tensor) or isinstance(b, torch.Tensor):
        if not (isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor)):
            return f"{path}: {type(a).__name__} against {type(b).__name__}"
        if a.dtype != b.dtype or a.shape != b.shape:
            return f"{path}: {a.dtype} {tuple(a.shape)} against {b.dtype} {tuple(b.shape)}"
        if torch.equal(bits(a), bits(b)):
            return None
        return f"{path}: {int((bits(a) != bits(b)).sum())} of {a.numel()} elements differ"
    if isinstance(a, dict) and isinstance(b, dict):
        if list(a) != list(b):
            return f"{path}: keys {sorted(set(a) ^ set(b)) or 'in another order'}"
        for k in a:
            d = _diff(a[k], b[k], f"{path}[{k!r}]")
            if d:
                return d
        return None
    if isinstance(a, (list, tuple)) and isinstance(b, (list, tuple)):
        if type(a) is not type(b) or len(a) != len(b):
            return f"{path}: {type(a).__name__} of {len(a)} against {type(b).__name__} of {len(b)}"
        for i, (x, y) in enumerate(zip(a, b)):
            d = _diff(x, y, f"{path}[{i}]")
            if d:
                return d
        return None
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return None if np.array_equal(a, b) else f"{path}: arrays differ"
    return None if type(a) is type(b) and a == b else f"{path}: {a!r} against {b!r}"


# what a checkpoint holds of the run, in the order it is compared; `args` is not among them (the output directory and --resume differ by design).
# optimizer: the moments of the tail's state_keys and `ema` by their bits, `step`, `lr` and the tail's name by ==
CHECKPOINT_KEYS = ("epoch", "lr_scheduler", "optimizer", "model", "model_ema", "data", "max_accuracy")


def checkpoint_diff(a, b, keys=CHECKPOINT_KEYS):
    for k in keys:
        if (k in a) != (k in b):
            return f"{k!r}: held by one checkpoint only"
        if k in a:
            d = _diff(a[k], b[k], k)
            if d:
                return d
    if "rng" in a and "rng" in b:       # the streams the next step would draw from (Python's is drawn from by no step and reseeded by no run)
        for k in ("torch", "device", "numpy"):
            d = _diff(a["rng"].get(k), b["rng"].get(k), f"rng[{k!r}]")
            if d:
                return d
    return None


def same_checkpoint(a, b, where=""):
    d = checkpoint_diff(a, b)
    assert d is None, where + d
    return True


def test_same_checkpoint_sees_one_bit_and_ignores_args():
    t = torch.arange(12, dtype=torch.float32).reshape(3, 4)
    ck = lambda: {"model": {"w": t.clone(), "b": t[0].to(torch.bfloat16)}, "model_ema": {"w": t.clone()},
                  "optimizer": {"ema": t.clone(), "step": 3, "lr": 1e-5, "m": t.clone(), "v": t.clone()},
                  "lr_scheduler": {"last": 0}, "epoch": 0, "args": argparse.Namespace(output_dir=object())}
    a, b = ck(), ck()
    assert same_checkpoint(a, b)
    b["optimizer"]["v"].view(torch.int32)[1, 2] ^= 1            # the last mantissa bit of one second moment
    assert checkpoint_diff(a, b) == "optimizer['v']: 1 of 12 elements differ"
    b = ck()
    b["model"]["w"][0, 0] = -0.0                                # equal as floats, not as bits
    assert checkpoint_diff(a, b) == "model['w']: 1 of 12 elements differ"
    for key, val, said in (("step", 4, "optimizer['step']: 3 against 4"), ("lr", 2e-5, "optimizer['lr']: 1e-05 against 2e-05")):
        b = ck()
        b["optimizer"][key] = val
        assert checkpoint_diff(a, b) == said
    b = ck()
    b["lr_scheduler"]["last"], b["epoch"] = 1, 1
    assert checkpoint_diff(a, b) == "epoch: 0 against 1"
    b = ck()
    b["data"] = {"rng": (3, (1, 2), None), "drawn": 8}
    assert checkpoint_diff(a, b) == "'data': held by one checkpoint only"
    a["data"] = {"rng": (3, (1, 2), None), "drawn": 12}
    assert checkpoint_diff(a, b) == "data['drawn']: 12 against 8"
    with pytest.raises(AssertionError, match="data"):
        same_checkpoint(a, b)


# ---- the runs ---------------------------------------------------------------------------------------------------------------------------------

class Run:
    def __init__(self, args):
        self.args, self.dir, self._loaded = args, os.path.join(args.output_dir, f"sub-dataset{args.start_division}"), {}

    def path(self, epoch):
        return os.path.join(self.dir, f"checkpoint_e{epoch}.pth")

    def checkpoint(self, epoch):
        """the checkpoint written after `epoch`, mapped from its file once (the moments, the EMA and the weights are 430 MB)"""
        if epoch not in self._loaded:
            self._loaded[epoch] = torch.load(self.path(epoch), map_location="cpu", weights_only=False, mmap=True)
        return self._loaded[epoch]

    def log(self):
        with open(os.path.join(self.dir, "log.txt")) as f:
            return [json.loads(line) for line in f.read().splitlines()]


def run_main(flags, out, keep=(0, 1, 2)):
    """distill_sub.main(flags) into `out`; every checkpoint_temp.pth of an epoch in `keep` is also kept as checkpoint_e{epoch}.pth: a second
    name of the same file where the file system has them (every epoch then writes a new checkpoint_temp.pth), a copy elsewhere"""
    import distill_sub
    from devit_amd import utils
    args = argparse.ArgumentParser(parents=[distill_sub.get_args_parser()]).parse_args(list(flags) + ["--output_dir", str(out)])
    real = utils.save_on_master

    def save_and_keep(obj, path, *a, **k):
        path = str(path)
        per_epoch = os.path.basename(path) == "checkpoint_temp.pth"
        if per_epoch and os.path.exists(path):
            os.unlink(path)
        real(obj, path, *a, **k)
        if per_epoch and obj["epoch"] in keep:
            kept = os.path.join(os.path.dirname(path), f"checkpoint_e{obj['epoch']}.pth")
            try:
                os.link(path, kept)
            except OSError:
                shutil.copyfile(path, kept)
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(utils, "save_on_master", save_and_keep)
        distill_sub.main(args)
    return Run(args)


def uninterrupted(flags, root):
    """run A and the control: A' gives A's bits after the first epoch and after the last"""
    A = run_main(flags, os.path.join(str(root), "a"))
    A2 = run_main(flags, os.path.join(str(root), "a2"), keep=(0, 2))
    for e in (0, 2):
        same_checkpoint(A.checkpoint(e), A2.checkpoint(e), f"control: two uninterrupted runs differ after epoch {e}: ")
    shutil.rmtree(A2.args.output_dir)
    return A


def check_continuation(A, flags, root):
    B = run_main(list(flags) + ["--resume", A.path(0)], os.path.join(str(root), "b"), keep=(1, 2))
    assert B.args.start_epoch == 1
    same_checkpoint(A.checkpoint(1), B.checkpoint(1), "after epoch 1, the resumed run's first: ")
    assert checkpoint_diff(A.checkpoint(0), B.checkpoint(1), keys=("model",)) is not None         # the resumed run trained
    same_checkpoint(A.checkpoint(2), B.checkpoint(2), "after epoch 2: ")
    la, lb = A.log(), B.log()
    assert [l["epoch"] for l in la] == [0, 1, 2] and [l["epoch"] for l in lb] == [1, 2]
    for x, y in zip(la[1:], lb):
        assert sorted(x) == sorted(y)
        stats = [k for k in x if k.startswith(("train_", "test_"))]
        assert {"train_loss", "train_lr", "train_cls_loss", "test_loss", "test_acc1", "test_acc5"} <= set(stats)
        for k in stats:
            assert x[k] == y[k], (x["epoch"], k, x[k], y[k])
    return B


@pytest.fixture(scope="module")
def default_run(dev, tmp_path_factory):
    """run A of the common flags alone (and its control), shared by the `default` case and the --resume --eval test"""
    root = tmp_path_factory.mktemp("default")
    yield uninterrupted(COMMON, root), root
    shutil.rmtree(root, ignore_errors=True)


@pytest.fixture(scope="module")
def image_tree(tmp_path_factory):
    """the image folders and the teacher file of tests/test_gpu_augment.py::test_distill_sub_cli_device_data"""
    Image = pytest.importorskip("PIL.Image")
    import devit_amd
    src = dict(np.load(os.path.join(ROOT, "tests", "golden", "augment_pil.npz")))["src32"]
    top = tmp_path_factory.mktemp("tree")
    root = top / "data" / "sub-dataset0"
    for split, n in (("train_dataset", 260), ("test_dataset", 6)):
        for i in range(n):
            d = root / split / f"class{i % 5}"
            d.mkdir(parents=True, exist_ok=True)
            Image.fromarray(np.roll(src[i % 4], i, axis=1)).save(d / f"{i:04d}.png")
    tdir = top / "teacher" / "sub-dataset0"
    tdir.mkdir(parents=True)
    torch.manual_seed(0)
    torch.save(devit_amd.create_model("deit_base_distilled_patch16_224", num_classes=5, img_size=48).state_dict(), tdir / "checkpoint.pth")
    return top


CASES = {
    "default": [],                                                      # Mixup 0.8 / CutMix 1.0 in batch mode, drop-path 0.1
    "drop": ["--drop", "0.1"],
    "elem": ["--mixup-mode", "elem", "--cutmix-minmax", "0.2", "0.8"],
    "nomix": ["--mixup", "0", "--cutmix", "0", "--drop-path", "0"],
    **{f"opt-{name}": ["--opt", name] for name in optim.OPT_NAMES if name != "adamw"},
    "device-data": None,
    "full-size": None,
}


@pytest.mark.parametrize("case", list(CASES))
def test_resumed_run_continues_bit_for_bit(case, dev, tmp_path, request):
    """On the parent commit, whose checkpoints held no random stream, `nomix` passed and every other case differed after the resumed run's first
    epoch, first in optimizer['ema'] (2.1 to 4.4 million of 21.6 million elements; 55 to 57 thousand under momentum and nesterov; 14 million with
    --device-data); the control held in all of them."""
    if case == "default":
        A, root = request.getfixturevalue("default_run")
        flags = COMMON
    else:
        root = tmp_path
        if case == "device-data":
            tree = request.getfixturevalue("image_tree")
            flags = common(synthetic=0, size=48, batch=64, division=20) + ["--device-data", "--device-aug", "--aa", "rand-m9-mstd0.5-inc1-n2", "--data-path", str(tree / "data"), "--teacher-path",
                      str(tree / "teacher"), "--eval-batch-size", "4", "--reprob", "0.5", "--recount", "2", "--train-interpolation", "random"]
        elif case == "full-size":
            flags = common(synthetic=2, size=224)
        else:
            flags = COMMON + CASES[case]
        A = uninterrupted(flags, root)
    try:
        B = check_continuation(A, flags, root)
        if case == "device-data":                      # four batches of 64 per epoch off the private stream, carried over the resume
            assert [A.checkpoint(e)["data"]["drawn"] for e in (0, 2)] == [256, 768] and B.checkpoint(2)["data"]["drawn"] == 768
        if case.startswith("opt-"):
            assert B.checkpoint(2)["optimizer"]["opt"] == case[4:]
    finally:
        shutil.rmtree(os.path.join(str(root), "b"), ignore_errors=True)
        if case != "default":
            shutil.rmtree(os.path.join(str(root), "a"), ignore_errors=True)


def test_resume_eval_gives_the_logged_scores(default_run, tmp_path, capsys):
    """--resume <checkpoint> --eval evaluates the weights the checkpoint holds: the scores the run logged for that epoch, to the bit"""
    A, _ = default_run
    import distill_sub
    args = argparse.ArgumentParser(parents=[distill_sub.get_args_parser()]).parse_args(
        COMMON + ["--resume", A.path(1), "--eval", "--output_dir", str(tmp_path / "ev")])
    capsys.readouterr()
    distill_sub.main(args)
    printed = [l for l in capsys.readouterr().out.splitlines() if l.startswith("{'loss'")]
    assert len(printed) == 1, printed
    got, logged = ast.literal_eval(printed[0]), A.log()[1]
    assert logged["epoch"] == 1 and sorted(got) == ["acc1", "acc5", "loss"]
    for k in ("loss", "acc1", "acc5"):
        assert got[k] == logged[f"test_{k}"], (k, got[k], logged[f"test_{k}"])
    assert not os.path.exists(os.path.join(args.output_dir, "sub-dataset0", "log.txt"))


class _CutOff(Exception):
    """the job is cut off (raised by the scripted evaluation)"""


@pytest.mark.parametrize("script,replaced", [((50.0, 30.0), False), ((30.0, 50.0), True)])
def test_best_model_survives_a_resume(script, replaced, dev, tmp_path, monkeypatch):
    """The best accuracy so far travels in the checkpoint: a run resumed into its own directory replaces checkpoint.pth (which ensemble.py reads)
    only with a better model.  evaluate is scripted (as in tests/test_shrink_search.py): script[0] for epoch 0, then the job is cut off, and
    script[1] for epoch 1 of the resumed run.  Both runs ask for two epochs: the directory's name holds --epochs."""
    from devit_amd import engine
    answers = iter([script[0], _CutOff, script[1]])

    def scripted(loader, model, device):
        a = next(answers)
        if a is _CutOff:
            raise _CutOff
        return {"loss": 1.0, "acc1": a, "acc5": 60.0}
    monkeypatch.setattr(engine, "evaluate", scripted)
    flags = common(synthetic=1, epochs=2)
    import distill_sub
    args = argparse.ArgumentParser(parents=[distill_sub.get_args_parser()]).parse_args(flags + ["--output_dir", str(tmp_path)])
    with pytest.raises(_CutOff):
        distill_sub.main(args)
    out = os.path.join(args.output_dir, "sub-dataset0")
    best, temp, result = (os.path.join(out, n) for n in ("checkpoint.pth", "checkpoint_temp.pth", "result.txt"))
    digest = lambda: hashlib.sha256(open(best, "rb").read()).hexdigest()
    before = digest()
    ck = torch.load(temp, map_location="cpu", weights_only=False)
    assert ck["epoch"] == 0 and ck["max_accuracy"] == script[0] and open(result).read() == f"Final Accuracy: {script[0]}\n"
    second = run_main(flags + ["--resume", temp], tmp_path, keep=())
    assert second.dir == out and [l["epoch"] for l in second.log()] == [0, 1] and next(answers, None) is None
    assert (digest() != before) == replaced
    assert open(result).read() == "Final Accuracy: 50.0\n"
    ck = torch.load(temp, map_location="cpu", weights_only=False)
    assert ck["epoch"] == 1 and ck["max_accuracy"] == 50.0
