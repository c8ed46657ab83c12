"""What --resume carries beside the weights, checked without a device: the global random streams of utils.rng_state() go through a checkpoint
file and continue where they stopped, a checkpoint from before they were kept loads as it always did, and the two CLIs that inherit
--resume without implementing it refuse it."""
import argparse
import io
import random

import numpy as np
import pytest
import torch


def _through_a_file(obj):
    """torch.save / torch.load as distill_sub.py does them (the checkpoint holds an argparse Namespace, hence weights_only=False)"""
    buf = io.BytesIO()
    torch.save(obj, buf)
    buf.seek(0)
    return torch.load(buf, map_location="cpu", weights_only=False)


def _draws(n):
    """n rounds over every stream a training step draws from, by the calls that draw from them; everything as plain Python values"""
    import distill_sub
    from devit_amd import de_vit
    batch = distill_sub.Mixup(0.8, 1.0, 1.0, 0.5, 0.1, 25, img_size=64)
    minmax = distill_sub.Mixup(0.8, 1.0, 1.0, 0.5, 0.1, 25, cutmix_minmax=(0.2, 0.8), img_size=64)
    elem = distill_sub.Mixup(0.8, 1.0, 1.0, 0.5, 0.1, 25, mode="elem", cutmix_minmax=(0.2, 0.8), img_size=64)
    pair = distill_sub.Mixup(0.8, 1.0, 1.0, 0.5, 0.1, 25, mode="pair", img_size=64)
    out = []
    for _ in range(n):
        out.append(("torch.rand", torch.rand(3).tolist()))
        out.append(("dropout seed", de_vit.draw_dropout_seed()))
        out.append(("np.beta", float(np.random.beta(0.8, 0.8))))
        out.append(("np.rand", np.random.rand(2).tolist()))
        out.append(("np.randint", int(np.random.randint(64))))
        out.append(("random.random", random.random()))
        out.append(("Mixup.draw", batch.draw(64, 64)))
        out.append(("Mixup.draw minmax", minmax.draw(64, 64)))
        out.append(("draw_table elem", elem.draw_table(4, 64, 64).tobytes()))
        out.append(("draw_table pair", pair.draw_table(4, 64, 64).tobytes()))
    return out


@pytest.mark.parametrize("k,n", [(0, 4), (3, 5)])
def test_streams_continue_through_a_checkpoint(k, n):
    from devit_amd import utils
    torch.manual_seed(11)
    np.random.seed(12)
    random.seed(13)
    _draws(k)
    saved = _through_a_file({"rng": utils.rng_state("cpu")})["rng"]
    assert "device" not in saved                          # no generator but the host's was asked for
    want = _draws(n)
    moved = _draws(n)
    for name in ("torch.rand", "dropout seed", "np.beta", "np.rand", "random.random"):     # every stream did move on
        assert [w for w in want if w[0] == name] != [m for m in moved if m[0] == name], name
    assert utils.load_rng_state(saved, "cpu") is True
    got = _draws(n)
    for i, (w, g) in enumerate(zip(want, got)):
        assert w == g, (i, w[0])
    # the whole of it, again, after other draws: restoring is not a one-off
    torch.rand(7), np.random.rand(5), random.random()
    assert utils.load_rng_state(saved) is True            # (no device named: the current one, none here)
    assert _draws(n) == want


def test_each_stream_is_its_own_entry():
    """Dropping one entry from the state leaves exactly that stream where it was: every stream of the step has its own entry"""
    from devit_amd import utils
    torch.manual_seed(1)
    np.random.seed(2)
    random.seed(3)
    saved = utils.rng_state("cpu")
    assert set(saved) == {"torch", "numpy", "python"}
    first = (torch.rand(2).tolist(), np.random.rand(2).tolist(), random.random())
    for j, key in enumerate(("torch", "numpy", "python")):
        other = _through_a_file(saved)
        torch.manual_seed(21), np.random.seed(22), random.seed(23)
        fresh = {"torch": torch.get_rng_state(), "numpy": np.random.get_state(), "python": random.getstate()}
        other[key] = fresh[key]
        utils.load_rng_state(other, "cpu")
        again = (torch.rand(2).tolist(), np.random.rand(2).tolist(), random.random())
        assert [a == b for a, b in zip(first, again)] == [i != j for i in range(3)], key


def test_state_without_a_device_entry_and_old_checkpoints(capsys):
    import distill_sub
    from devit_amd import utils
    torch.manual_seed(5)
    np.random.seed(6)
    random.seed(7)
    state = _through_a_file(utils.rng_state("cpu"))
    want = _draws(2)
    # a state saved where there was no device generator, loaded for a device: the host streams come back, nothing else is asked for
    assert "device" not in state and utils.load_rng_state(state, "cuda") is True
    assert _draws(2) == want
    # a checkpoint written before the streams and the best accuracy were kept: nothing moves, one line says so, the best accuracy is 0.0
    old = _through_a_file({"model": {}, "optimizer": {}, "lr_scheduler": {"last": 0}, "epoch": 0, "model_ema": None, "scaler": {},
                           "args": argparse.Namespace(seed=0)})
    before = _through_a_file(utils.rng_state("cpu"))
    capsys.readouterr()
    assert utils.load_rng_state(old.get("rng"), "cpu") is False
    assert distill_sub.load_run_state(old, "cpu") == 0.0
    printed = capsys.readouterr().out
    assert printed.count("\n") == 1 and "restart from --seed" in printed
    after = utils.rng_state("cpu")
    assert torch.equal(before["torch"], after["torch"]) and before["python"] == after["python"]
    assert before["numpy"][0] == after["numpy"][0] and np.array_equal(before["numpy"][1], after["numpy"][1]) \
        and before["numpy"][2:] == after["numpy"][2:]
    # a new one: the streams and the accuracy come back, and nothing is printed
    new = _through_a_file({"rng": state, "max_accuracy": 37.5})
    assert distill_sub.load_run_state(new, "cpu") == 37.5 and capsys.readouterr().out == ""
    assert _draws(2) == want


@pytest.mark.parametrize("script", ["train_subdata", "ensemble"])
def test_resume_is_refused_where_it_is_not_implemented(script, monkeypatch):
    """Both CLIs inherit --resume from distill_sub.py's parser and restore nothing from it: main() refuses the flag before anything else runs."""
    import importlib
    import distill_sub
    mod = importlib.import_module(script)
    parse = argparse.ArgumentParser(parents=[mod.get_args_parser()], conflict_handler="resolve").parse_args
    args = parse(["--resume", "some/checkpoint_temp.pth", "--eval"])
    with pytest.raises(SystemExit) as e:
        distill_sub.check_no_resume(args, script + ".py")
    assert "--resume some/checkpoint_temp.pth" in str(e.value) and "distill_sub.py only" in str(e.value) and script + ".py" in str(e.value)
    distill_sub.check_no_resume(parse([]), script + ".py")               # without the flag: nothing
    # main() makes that check, and makes it first: before check_supported and before any device work
    reached = []
    monkeypatch.setattr(distill_sub, "check_supported", lambda a: reached.append("check_supported"))
    with pytest.raises(SystemExit) as e:
        mod.main(parse(["--resume", "some/checkpoint_temp.pth", "--device", "cpu"]))
    assert "distill_sub.py only" in str(e.value) and reached == []
