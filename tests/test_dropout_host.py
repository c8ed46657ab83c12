"""CPU-side checks of dropout p > 0: the numpy Philox4x32-10 that the GPU tests hold the kernels to reproduces the published known answers, the
host's threshold is the header's statement, and the probabilities are validated."""
import numpy as np
import pytest

import _philox as PH


def words(ctr, key):
    return " ".join("%08x" % int(w) for w in PH.philox4x32_10([np.uint32(c) for c in ctr], key))


def test_philox_known_answers():
    """Random123 kat_vectors, philox4x32 10 rounds"""
    assert words((0, 0, 0, 0), (0, 0)) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    f = 0xFFFFFFFF
    assert words((f, f, f, f), (f, f)) == "408f276d 41c83b0e a20bc7c6 6d5451fd"
    assert words((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0)) == "d16cfe09 94fdcceb 5001e420 24126ea1"


def test_mirror_counter_layout_and_keep_fraction():
    """element e = row * pitch + col: word e & 3 of counter (e >> 2, site, block); the mirror's keep fraction over 2^20 elements of seed 20240807,
    site 0, block 0 is within 5 sigma of a binomial (the bars the GPU test holds the kernel to)"""
    seed, thr = 20240807, PH.threshold(0.1)
    w = PH.philox4x32_10((np.uint32(5), np.uint32(0), np.uint32(2), np.uint32(7)), (seed & 0xFFFFFFFF, seed >> 32))
    m = PH.keep_mask(seed, 2, 7, thr, 3, 12, 12)                       # elements 20..23 = row 1, columns 8..11
    assert [bool(x) for x in m[1, 8:12]] == [int(x) >= thr for x in w]
    assert np.array_equal(PH.keep_mask(seed, 2, 7, thr, 3, 10, 12), m[:, :10])      # cols < pitch: the same elements
    for p, bar in ((0.1, 1.5e-3), (0.5, 2.5e-3)):
        frac = PH.keep_mask(seed, 0, 0, PH.threshold(p), 1024, 1024, 1024).mean()
        assert abs(frac - (1 - p)) <= bar, (p, frac)


def test_threshold_is_the_header_s_statement():
    from devit_amd import dropout
    assert dropout.threshold(0.0) == (0, 1.0)
    assert dropout.threshold(0.5) == (1 << 31, 2.0)
    thr, s = dropout.threshold(0.1)
    assert thr == int(np.floor(np.float64(0.1) * 2.0 ** 32)) == PH.threshold(0.1) and s == 1.0 / 0.9
    assert dropout.threshold(1.0 - 2.0 ** -40)[0] == 2 ** 32 - 1          # the largest threshold a p < 1 reaches


@pytest.mark.parametrize("p", [1.0, -0.1, 1.5, float("nan")])
def test_p_outside_the_half_open_unit_interval_raises(p):
    from devit_amd import dropout
    with pytest.raises(ValueError):
        dropout.threshold(p)


def test_model_with_rates_constructs_and_carries_them():
    import devit_amd
    m = devit_amd.create_model("dedeit", drop_rate=0.1, attn_drop_rate=0.1)
    assert m.pos_drop.p == 0.1 and m.dropout_seed is None and len(m.blocks) == 12
    for b in m.blocks:
        assert b.mlp.drop.p == 0.1 and b.attn.proj_drop.p == 0.1 and b.attn.attn_drop.p == 0.1


@pytest.mark.parametrize("kw", [dict(drop_rate=1.0), dict(drop_rate=-0.1), dict(attn_drop_rate=1.0), dict(attn_drop_rate=-0.5)])
def test_models_refuse_a_probability_outside_the_interval(kw):
    import devit_amd
    with pytest.raises(ValueError):
        devit_amd.create_model("dedeit", depth=1, num_classes=10, **kw)
    from devit_amd.de_vit import Attention, Mlp
    with pytest.raises(ValueError):
        Mlp(384, 1536, drop=1.0)
    with pytest.raises(ValueError):
        Attention(384, 6, proj_drop=1.0)


@pytest.mark.parametrize("cli", ["distill_sub", "train_subdata", "ensemble", "shrink"])
def test_cli_support_check_accepts_drop(cli):
    """--drop 0.1 parses in all four CLIs and passes the support check the three training CLIs share; each hands args.drop to its models"""
    import importlib
    import inspect
    import distill_sub
    mod = importlib.import_module(cli)
    args, _ = mod.get_args_parser().parse_known_args(["--drop", "0.1"])
    assert args.drop == 0.1
    if hasattr(args, "opt") and hasattr(args, "sched"):
        distill_sub.check_supported(args)
    assert "args.drop" in inspect.getsource(mod)
