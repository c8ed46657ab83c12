"""Host logic of the ensemble stage on the flat fused path, no GPU: EnsLoss's loss types, ddp.FlatParams / optim.FlatAdamW's decay mask over a
MultiViT, the reducer's bucket plan with (backbone, kind, block) report groups, the unchanged plan of a single VisionTransformer, the CLI flags,
and the float64 statement of the token KL loss (tests/_ens_model.py) against torch's own nn.KLDivLoss."""
import argparse

import pytest
import torch

import _ens_model as E
from devit_amd import ddp, losses, optim
from devit_amd.ensemble_models import MultiViT


def test_ens_loss_types():
    base = losses.SoftTargetCrossEntropy()
    for lt in ("mse", "kldiv"):
        assert losses.EnsLoss(base, None, "dedeit", "hard", 0.5, 1.0, loss_type=lt).loss_type == lt
    assert losses.EnsLoss(base, None, "devit", "hard", 0.5, 1.0, "kldiv").loss_type == "kldiv"
    with pytest.raises(NotImplementedError):
        losses.EnsLoss(base, None, "dedeit", "hard", 0.5, 1.0, loss_type="l1")


@pytest.fixture(scope="module")
def multi_flat():
    torch.manual_seed(0)
    multi = MultiViT("dedeit", num_div=2, num_classes_list=[5, 5])
    return multi, ddp.FlatParams(multi)


def test_flat_params_over_multivit(multi_flat):
    import ensemble
    multi, flat = multi_flat
    named = dict(multi.named_parameters())
    assert sorted(flat.names) == sorted(named) and flat.names[0].startswith("backbones.1.") and flat.names[-1].startswith("backbones.0.")
    lo, hi = flat.flat.data_ptr(), flat.flat.data_ptr() + 4 * flat.numel
    for name, p, o in zip(flat.names, flat.params, flat.offsets):
        assert p is named[name]
        assert p.data.data_ptr() == lo + 4 * o and p.data_ptr() + 4 * p.numel() <= hi               # aliases the flat master ...
        assert p.grad is not None and p.grad.data_ptr() == flat.flat_grad.data_ptr() + 4 * o       # ... and the flat gradient
    flat.flat_grad[flat.offsets[3]] = 7.0
    assert float(flat.params[3].grad.reshape(-1)[0]) == 7.0
    flat.flat_grad.zero_()
    opt = optim.FlatAdamW(flat, weight_decay=0.05, no_decay=optim.no_decay_names(multi))
    groups = ensemble.param_groups(multi, 0.05)
    assert groups[0]["weight_decay"] == 0.05 and groups[1]["weight_decay"] == 0.0
    exempt = {id(p) for p in groups[1]["params"]}
    assert {id(p) for g in groups for p in g["params"]} == {id(p) for p in flat.params}
    mask = opt.no_decay4.cpu()
    want = torch.zeros_like(mask)
    for name, p, o in zip(flat.names, flat.params, flat.offsets):
        if id(p) in exempt:
            want[o // 4:(o + p.numel() + 3) // 4] = 1
        # every granule of a tensor carries the tensor's own flag: no granule is shared between two tensors
        assert bool((mask[o // 4:(o + p.numel() + 3) // 4] == (1 if id(p) in exempt else 0)).all()), name
    assert torch.equal(mask, want)
    flag = lambda n: int(mask[flat.offsets[flat.names.index(n)] // 4])
    assert flag("backbones.0.pos_embed") == 0 and flag("backbones.1.cls_token") == 0 and flag("backbones.0.dist_token") == 0    # decayed: no no_weight_decay()
    assert flag("backbones.1.blocks.0.norm1.weight") == 1 and flag("backbones.0.blocks.3.mlp.fc1.bias") == 1
    assert flag("backbones.1.blocks.0.attn.qkv.weight") == 0


class _RecComm:
    """a recording stand-in for RcclComm: which element ranges of flat_grad were handed to the collective, in launch order"""

    def __init__(self, flat):
        self.world, self.base, self.ranges = 2, flat.flat_grad.data_ptr(), []

    def all_reduce(self, view, stream=None):
        s = (view.data_ptr() - self.base) // 4
        self.ranges.append((s, s + view.numel()))


def _backward_order(multi):
    """the parameter lists the autograd nodes report, in backward order: backbone 1 first -- final norm (the backbones have no heads), blocks
    11 .. 0, embeddings -- then backbone 0"""
    out = []
    for m in reversed(list(multi.backbones)):
        out.append(list(m.norm.parameters()))
        out += [list(b.parameters()) for b in reversed(list(m.blocks))]
        out.append([m.cls_token, m.dist_token, m.pos_embed] + list(m.patch_embed.parameters()))
    return out


@pytest.mark.parametrize("bucket_bytes", [25 << 20, 8 << 20, 1 << 20])
def test_reducer_plan_over_multivit(multi_flat, bucket_bytes):
    multi, flat = multi_flat
    comm = _RecComm(flat)
    red = ddp.BucketedGradReducer(flat, bucket_bytes=bucket_bytes, comm=comm).attach(multi)
    assert all(m.grad_ready is multi.backbones[0].grad_ready and m.grad_ready.reducer is red for m in multi.backbones)
    assert ddp._report_group("backbones.1.blocks.7.mlp.fc1.weight") == (1, 1, 7) and ddp._report_group("backbones.0.pos_embed") == (0, 2, 0)
    assert ddp._report_group("backbones.1.norm.bias") == (1, 0, 0) and ddp._report_group("blocks.7.mlp.fc1.weight") == (1, 7)
    for s, e, p0, p1 in red.buckets:
        assert len({flat.names[i].split(".")[1] for i in range(p0, p1 + 1)}) == 1, "a bucket spans two backbones"
        groups = [ddp._report_group(flat.names[i]) for i in range(p0, p1 + 1)]
        before = ddp._report_group(flat.names[p0 - 1]) if p0 else None
        after = ddp._report_group(flat.names[p1 + 1]) if p1 + 1 < len(flat.names) else None
        assert groups[0] != before and groups[-1] != after, "a bucket boundary inside a report group"
    assert len(red.buckets) >= 2 * 4                 # per backbone at least: norm + last block, middle blocks, block 0, embeddings
    reports = _backward_order(multi)
    for params in reports:
        multi.backbones[0].grad_ready(params)
    assert sorted(red.launch_order) == list(range(len(red.buckets))) and len(comm.ranges) == len(red.buckets)       # every bucket exactly once
    assert red.launch_order == list(range(len(red.buckets)))                                                      # ... and in flat order
    tiles = sorted(comm.ranges)
    assert tiles[0][0] == 0 and tiles[-1][1] == flat.numel and all(a[1] == b[0] for a, b in zip(tiles, tiles[1:]))
    with pytest.raises(RuntimeError):
        red.mark_ready(reports[3])                   # a double report
    assert red.finish() == list(range(len(red.buckets))) and flat.grad_scale == 0.5
    assert len(comm.ranges) == len(red.buckets)      # finish() had nothing left to launch
    flat.grad_scale = 1.0
    # an unreported bucket (the whole fusion head, which no autograd node reports) leaves at finish()
    from devit_amd.ensemble_models import EnsMLP
    ens_flat = ddp.FlatParams(EnsMLP("dedeit", 10, 384, [5, 5], 768))
    ens_comm = _RecComm(ens_flat)
    ens_red = ddp.BucketedGradReducer(ens_flat, comm=ens_comm)
    assert len(ens_red.buckets) == 1 and ens_red.finish() == [0] and ens_comm.ranges == [(0, ens_flat.numel)]


def _buckets_by_the_single_model_rule(flat, bucket_bytes):
    """the bucket rule as it stood before report groups knew about backbones, restated for one VisionTransformer: cut at the end of a report
    group when it is heads + norm + the last block, when the embeddings or block 0 come next, or when the next block would overflow the bucket"""
    def group(name):
        if name.startswith("blocks."):
            return (1, int(name.split(".")[1]))
        return (2, 0) if name.startswith(("patch_embed", "pos_embed", "cls_token", "dist_token")) else (0, 0)
    groups = [group(n) for n in flat.names]
    n = len(groups)
    end_of = lambda i: flat.offsets[i + 1] if i + 1 < n else flat.numel
    first_block = next(g for g in groups if g[0] == 1)
    final_block = next(g for g in reversed(groups) if g[0] == 1)
    out, start, last, limit = [], 0, 0, bucket_bytes // 4
    for i in range(n):
        end = end_of(i)
        if i + 1 < n and groups[i + 1] == groups[i]:
            continue
        nxt = groups[i + 1] if i + 1 < n else None
        size_next = sum(end_of(j) - flat.offsets[j] for j in range(i + 1, n) if groups[j] == nxt)
        if (nxt is None or groups[i] == first_block or nxt[0] == 2 or nxt == final_block
                or (groups[i][0] == 1 and end - start + size_next > limit)):
            out.append((start, end, last, i))
            start, last = end, i + 1
    return out


@pytest.mark.parametrize("bucket_bytes", [25 << 20, 8 << 20])
def test_single_model_buckets_unchanged(bucket_bytes):
    import devit_amd
    flat = ddp.FlatParams(devit_amd.create_model("dedeit", num_classes=25))
    red = ddp.BucketedGradReducer(flat, bucket_bytes=bucket_bytes, world=2)
    assert red.buckets == _buckets_by_the_single_model_rule(flat, bucket_bytes)
    assert len(red.buckets) == {25 << 20: 7, 8 << 20: 13}[bucket_bytes]


def test_cli_flags():
    import ensemble
    parse = argparse.ArgumentParser(parents=[ensemble.get_args_parser()], conflict_handler="resolve").parse_args
    a = parse([])
    assert a.torch_optim is False and a.loss == "mse" and a.model_ema is True and a.model_ema_decay == 0.99996
    a = parse(["--torch-optim", "--loss", "kldiv", "--no-model-ema", "--model-ema-force-cpu", "--gates", "g.pt", "--physical-shrink"])
    assert a.torch_optim and a.loss == "kldiv" and a.model_ema is False and a.model_ema_force_cpu and a.physical_shrink


@pytest.mark.parametrize("n,batch", E.kldiv_cases())
def test_kldiv_statement_is_torchs(n, batch):
    """_ens_model.kldiv_ref is nn.KLDivLoss(reduction="batchmean", log_target=True) in float64, loss and gradient; the loss bound stands on
    sum |term|, never below the same count on |loss|"""
    i = E.kldiv_inputs(n, batch)
    s = i["s"].to(torch.float64).view(batch, -1).requires_grad_(True)
    t = i["t"].to(torch.float64).view(batch, -1)
    loss = torch.nn.KLDivLoss(reduction="batchmean", log_target=True)(s, t)
    loss.backward()
    ref, bnd = E.kldiv_bounds(i["s"], i["t"], batch)
    assert abs(float(loss.detach()) - float(ref["loss"])) <= 1e-12 * float(bnd["loss"]) / E.U
    assert torch.allclose(s.grad.reshape(-1), ref["ds"], rtol=1e-13, atol=0)
    assert float(bnd["loss"]) >= E.U * 30 * abs(float(ref["loss"])) and bool((bnd["ds"] > 0).all())
