"""The shrink stage without a GPU: the ranking kernels' C ABI is declared, bound and exported; the candidate screen keeps the
reference's 2 % window on the model's own geometry; the shrink.py CLI takes the reference's flags, refuses a distributed
launch and writes the files distill_sub.py --shrink_checkpoint reads (the evaluator is a stub here; the search runs on
the GPU in tests/test_gpu_hsic.py)."""
import argparse
import inspect
import json
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT

HSIC_SYMBOLS = ("devit_hsic_target", "devit_hsic_scores_workspace", "devit_hsic_scores", "devit_hsic_head_pairs")
DEDEIT = dict(emb=384, head=6, layer=12, mlp_ratio=4)


def test_hsic_symbols_declared_bound_and_exported():
    from devit_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "devit_hip.h")).read(), flags=re.S)
    exported = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    lib = _lib.load()
    for name in HSIC_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES, name
        assert re.search(r" T %s\b" % name, exported) and hasattr(lib, name), name
    assert lib.devit_version() == _lib.ABI_VERSION       # (the HSIC symbols were additive: they came without a new version)
    # the workspace query is host arithmetic: B rounded up to the 64-sample tile, fp32, one slice per unit and token
    assert lib.devit_hsic_scores_workspace(37, 198, 192) == 192 * 198 * 64 * 4
    assert lib.devit_hsic_scores_workspace(256, 198, 64) == 64 * 198 * 256 * 4
    assert lib.devit_hsic_scores_workspace(257, 198, 64) == 0 and lib.devit_hsic_scores_workspace(1, 198, 64) == 0


def test_hsic_entry_points_refuse_bad_arguments():
    """Argument checks run before any launch, so they can be exercised without a GPU: a batch outside 2..256 is refused
    loudly, never truncated."""
    import ctypes as C
    from devit_amd import _lib
    lib = _lib.load()
    fake = C.c_void_p(4096)                              # never dereferenced: the checks fail first
    for B in (1, 257, 1024):
        rc = lib.devit_hsic_scores(fake, _lib.HSIC_BF16, B, 198, 64, 1, 198 * 64, 64, fake, fake, None, None, fake, 1 << 40, None)
        assert rc == -2 and b"outside 2..256" in lib.devit_last_error(), (B, rc)
        assert lib.devit_hsic_target(fake, B, 10, 1, fake, fake, 1 << 40, None) == -2
        assert lib.devit_hsic_head_pairs(fake, 6, B, fake, None) == -2
    assert lib.devit_hsic_scores(fake, 7, 8, 198, 64, 1, 198 * 64, 64, fake, fake, None, None, fake, 1 << 40, None) == -2     # element type
    assert lib.devit_hsic_scores(fake, 0, 8, 198, 64, 1, 198 * 64, 32, fake, fake, None, None, fake, 1 << 40, None) == -2     # rows overlap
    assert lib.devit_hsic_scores(fake, 0, 8, 198, 64, 1, 198 * 64, 64, fake, fake, None, None, fake, 1024, None) == -2        # workspace
    assert lib.devit_hsic_scores(fake, 0, 8, 198, 6, 64, 198 * 384, 384, fake, fake, fake, None, fake, 1 << 40, None) == -2   # act with group > 1
    assert lib.devit_hsic_head_pairs(fake, 17, 8, fake, None) == -2 and lib.devit_hsic_head_pairs(fake, 1, 8, fake, None) == -2


def test_scores_keep_signatures_and_cpu_statement():
    from devit_amd import shrink
    assert list(inspect.signature(shrink.neuron_scores).parameters) == ["neuron_output", "prob"]
    assert list(inspect.signature(shrink.head_scores).parameters) == ["head_output", "prob"]
    sig = inspect.signature(shrink.rank_units)
    assert list(sig.parameters) == ["model", "data_loader", "device", "batches"] and sig.parameters["batches"].default == 1
    g = dict(np.load(os.path.join(GOLDEN, "imp_rank.npz")))          # CPU tensors: the torch statement, pinned to the golden ranks
    prob = torch.softmax(torch.from_numpy(g["logits"]), -1)
    assert np.array_equal(np.argsort(shrink.neuron_scores(torch.from_numpy(g["n1"]), prob).numpy()), g["neuron_rank"][1])


def test_screen_dedeit():
    from devit_amd import flops, shrink
    gold = json.load(open(os.path.join(GOLDEN, "flops.json")))
    assert shrink.dense_gflops(**DEDEIT) == gold["dedeit_dense_gflops"]
    target = shrink.macs_target(0.36, **DEDEIT)
    assert target == 0.36 * gold["dedeit_dense_gflops"]
    x = shrink.screen(target, 20, 0, 0.5, rng=np.random.default_rng(7), **DEDEIT)
    assert x.shape == (20, 24) and x.dtype == np.float64 and (x >= 0).all() and (x < 0.5).all()
    for row in x:
        macs = flops.macs_g(neuron_sparsity=row[:12], head_sparsity=row[12:], emb=384, head=6, layer=12, mlp_ratio=4)
        assert abs(macs - target) <= 0.02 * target, (macs, target)
    assert len({row.tobytes() for row in x}) == 20
    assert np.array_equal(x, shrink.screen(target, 20, 0, 0.5, rng=np.random.default_rng(7), **DEDEIT))
    assert not np.array_equal(x, shrink.screen(target, 20, 0, 0.5, rng=np.random.default_rng(8), **DEDEIT))
    # the chunked evaluation is flops.macs_g row by row
    r = np.random.default_rng(1).uniform(0, 0.5, (500, 24))
    rows = shrink._macs_g_rows(r, 12, emb=384, head=6, mlp_ratio=4)
    assert all(rows[i] == flops.macs_g(neuron_sparsity=q[:12], head_sparsity=q[12:], **DEDEIT) for i, q in enumerate(r))
    with pytest.raises(RuntimeError):                    # a target nothing meets ends with an error, not a spin
        shrink.screen(10.0 * target, 2, 0, 0.5, rng=np.random.default_rng(0), max_draws=4096, **DEDEIT)


REFERENCE_FLAGS = """--batch-size --eval-batch-size --epochs --output_dir --model --input-size --drop --drop-path --model-ema --no-model-ema
--model-ema-decay --model-ema-force-cpu --opt --opt-eps --opt-betas --clip-grad --momentum --weight-decay --sched --lr --lr-noise
--lr-noise-pct --lr-noise-std --warmup-lr --min-lr --decay-epochs --warmup-epochs --cooldown-epochs --patience-epochs --decay-rate --dr
--color-jitter --aa --smoothing --train-interpolation --repeated-aug --no-repeated-aug --reprob --remode --recount --resplit --mixup
--cutmix --cutmix-minmax --mixup-prob --mixup-switch-prob --mixup-mode --teacher-model --teacher-path --distillation-type
--distillation-alpha --distillation-tau --finetune --data-path --data-set --num_division --start-division --inat-category --resume
--start_epoch --device --seed --eval --dist-eval --num_workers --pin-mem --no-pin-mem --world_size --dist_url --neuron_shrinking
--head_shrinking --neuron_sparsity --head_sparsity --shrink_ratio --bound --population""".split()


def _parse(argv):
    import shrink as cli
    return argparse.ArgumentParser(parents=[cli.get_args_parser()]).parse_args(argv)


def test_cli_parser_takes_the_reference_flag_set():
    import shrink as cli
    known = {s for a in cli.get_args_parser()._actions for s in a.option_strings}
    assert set(REFERENCE_FLAGS) <= known, sorted(set(REFERENCE_FLAGS) - known)
    assert {"--synthetic", "--no-physical-shrink", "--rank-batches"} <= known
    d = _parse([])
    assert (d.batch_size, d.shrink_ratio, d.bound, d.population, d.rank_batches) == (2, 0.3, 0.5, 100, 1)
    assert d.physical_shrink and not d.neuron_shrinking and not d.head_shrinking and d.data_set == "cifar100" and d.num_division == 4
    a = _parse(["--shrink_ratio", "0.36", "--bound", "0.4", "--population", "7", "--neuron_shrinking", "--head_shrinking", "--data-set", "pets",
                "--finetune", "x.pth", "--resume", "y.pth", "--rank-batches", "3", "--no-physical-shrink", "--lr", "1e-3", "--aa", "none"])
    assert (a.shrink_ratio, a.bound, a.population, a.rank_batches, a.physical_shrink) == (0.36, 0.4, 7, 3, False)


def test_cli_refuses_a_distributed_launch(monkeypatch, tmp_path):
    import shrink as cli
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "0")
    with pytest.raises(SystemExit) as e:
        cli.main(_parse(["--synthetic", "1", "--device", "cpu", "--output_dir", str(tmp_path)]))
    assert "single process" in str(e.value)
    monkeypatch.delenv("WORLD_SIZE")
    monkeypatch.delenv("RANK")
    with pytest.raises(SystemExit):
        cli.main(_parse(["--synthetic", "1", "--device", "cpu", "--output_dir", str(tmp_path), "--world_size", "8"]))
    assert not os.listdir(tmp_path)


def test_cli_writes_what_distill_sub_reads(monkeypatch, tmp_path):
    """main() with both rankings switched off (natural order: nothing runs on a GPU) and a stubbed evaluator: the two files
    land where distill_sub.py --shrink_checkpoint looks and read_shrink_checkpoint returns the best candidate's ratios; the
    model the search worked on comes back with all-ones gates and no compacted weights."""
    import shrink as cli
    from devit_amd import engine, flops, shrink
    seen = []

    def fake_evaluate(loader, model, device):
        kept = [(int(b.attn.gate.sum()), int(b.mlp.gate.sum())) for b in shrink._blocks(model)]
        seen.append((model, kept))
        return {"acc1": [10.0, 30.0, 20.0][len(seen) - 1], "acc5": 50.0, "loss": 1.0}
    monkeypatch.setattr(engine, "evaluate", fake_evaluate)
    args = _parse(["--synthetic", "1", "--device", "cpu", "--batch-size", "2", "--population", "3", "--shrink_ratio", "0.36",
                   "--no-physical-shrink", "--output_dir", str(tmp_path), "--seed", "5"])
    xp, yp = cli.main(args)
    out = os.path.join(str(tmp_path), "cifar100_div4", "dedeit", "shrink")
    assert args.shrink_dir == out and sorted(os.listdir(out)) == ["shrinked_accuracy.npy", "shrinked_policy.npy"]
    assert xp.shape == (3, 24) and yp.tolist() == [10.0, 30.0, 20.0]
    ns, hs = shrink.read_shrink_checkpoint(out)
    assert np.array_equal(ns, xp[1, :12]) and np.array_equal(hs, xp[1, 12:])
    target = shrink.macs_target(0.36, **DEDEIT)
    assert np.array_equal(xp, shrink.screen(target, 3, 0, 0.5, rng=np.random.default_rng(5), **DEDEIT))
    # every candidate was evaluated MASKED with its own policy: kept counts are the reference's int(n * (1 - ratio))
    assert len(seen) == 3
    for (model, kept), row in zip(seen, xp):
        assert kept == [(int(6 * (1 - row[12 + i])), int(1536 * (1 - row[i]))) for i in range(12)]
        assert abs(flops.macs_g(neuron_sparsity=row[:12], head_sparsity=row[12:], **DEDEIT) - target) <= 0.02 * target
    model = seen[0][0]
    for blk in shrink._blocks(model):
        assert bool((blk.attn.gate == 1).all()) and bool((blk.mlp.gate == 1).all()) and getattr(blk, "_compact", None) is None
