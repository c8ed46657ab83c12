#!/usr/bin/env python3
"""shrink.py on MI355X: the policy search between train_subdata.py and distill_sub.py (reference shrink.py:406-418,
core/shrink_imp.py:66-82,138-179).

Ranks the neurons and heads of a trained sub-model on `--rank-batches` training batches (HSIC relevance / redundancy and
activation mass, devit_amd.shrink.rank_units on csrc/hsic.hip), screens `--population` random per-block sparsity vectors
whose analytic cost is `--shrink_ratio` of the dense model's, evaluates the model masked with each of them and writes

    <output_dir>/<data_set>_div<num_division>/<model>/shrink/shrinked_policy.npy     [population, 24]
    <output_dir>/<data_set>_div<num_division>/<model>/shrink/shrinked_accuracy.npy   [population]

-- the directory `distill_sub.py --shrink_checkpoint` takes.  The reference's script reads args.dataset, args.nb_classes and
args.classifier_choose, none of which its parser defines; here the class count comes from the data set and the division, and
the depth from the model.  Its whole flag set is accepted; the flags of the training loop it never enters are ignored.
`--synthetic N` and `--no-physical-shrink` as in distill_sub.py.  Single process: the search evaluates candidates one
after the other on one GPU.
"""
import argparse
import os
from pathlib import Path

import numpy as np
import torch

import devit_amd
from devit_amd import shrink as shrink_ops
from distill_sub import NUM_CLASSES, build_loaders, check_input_size


def get_args_parser():
    p = argparse.ArgumentParser('DeViT shrinking script (MI355X)', add_help=False)
    a = p.add_argument
    a('--batch-size', default=2, type=int); a('--eval-batch-size', default=512, type=int); a('--epochs', default=300, type=int)
    a('--output_dir', default='', help='path where to save, empty for no saving')
    a('--model', default='dedeit', type=str, metavar='MODEL'); a('--input-size', default=224, type=int)
    a('--drop', type=float, default=0.0); a('--drop-path', type=float, default=0.1)
    a('--model-ema', action='store_true'); a('--no-model-ema', action='store_false', dest='model_ema'); p.set_defaults(model_ema=True)
    a('--model-ema-decay', type=float, default=0.99996); a('--model-ema-force-cpu', action='store_true', default=False)
    a('--opt', default='adamw', type=str); a('--opt-eps', default=1e-8, type=float); a('--opt-betas', default=None, type=float, nargs='+')
    a('--clip-grad', type=float, default=None); a('--momentum', type=float, default=0.9); a('--weight-decay', type=float, default=0.05)
    a('--sched', default='cosine', type=str); a('--lr', type=float, default=5e-4)
    a('--lr-noise', type=float, nargs='+', default=None); a('--lr-noise-pct', type=float, default=0.67); a('--lr-noise-std', type=float, default=1.0)
    a('--warmup-lr', type=float, default=1e-6); a('--min-lr', type=float, default=1e-5); a('--decay-epochs', type=float, default=30)
    a('--warmup-epochs', type=int, default=5); a('--cooldown-epochs', type=int, default=10); a('--patience-epochs', type=int, default=10)
    a('--decay-rate', '--dr', type=float, default=0.1)
    a('--color-jitter', type=float, default=0.4); a('--aa', type=str, default='rand-m9-mstd0.5-inc1'); a('--smoothing', type=float, default=0.1)
    a('--train-interpolation', type=str, default='bicubic'); a('--repeated-aug', action='store_true')
    a('--no-repeated-aug', action='store_false', dest='repeated_aug'); p.set_defaults(repeated_aug=True)
    a('--reprob', type=float, default=0.25); a('--remode', type=str, default='pixel'); a('--recount', type=int, default=1)
    a('--resplit', action='store_true', default=False)
    a('--mixup', type=float, default=0.8); a('--cutmix', type=float, default=1.0); a('--cutmix-minmax', type=float, nargs='+', default=None)
    a('--mixup-prob', type=float, default=1.0); a('--mixup-switch-prob', type=float, default=0.5); a('--mixup-mode', type=str, default='batch')
    a('--teacher-model', default='regnety_160', type=str); a('--teacher-path', type=str, default='')
    a('--distillation-type', default='none', choices=['none', 'soft', 'hard'], type=str)
    a('--distillation-alpha', default=0.5, type=float); a('--distillation-tau', default=1.0, type=float)
    a('--finetune', default='', help='start from this checkpoint (its classifier is dropped when the class count differs)')
    a('--data-path', default=r'./dataset', type=str)
    a('--data-set', default='cifar100', choices=['cifar100', 'IMNET', 'cars', 'pets', 'flowers'], type=str)
    a('--num_division', metavar='N', type=int, default=4); a('--start-division', metavar='N', type=int, default=0)
    a('--inat-category', default='name')
    a('--resume', default='', help='the trained sub-model to shrink (a state dict, or a checkpoint holding one under "model")')
    a('--start_epoch', default=0, type=int); a('--device', default='cuda'); a('--seed', default=0, type=int)
    a('--eval', action='store_true'); a('--dist-eval', action='store_true', default=False); a('--num_workers', default=10, type=int)
    a('--pin-mem', action='store_true'); a('--no-pin-mem', action='store_false', dest='pin_mem'); p.set_defaults(pin_mem=True)
    a('--world_size', default=1, type=int); a('--dist_url', default='env://')
    a('--neuron_shrinking', action='store_true', default=False); a('--head_shrinking', action='store_true', default=False)
    a('--neuron_sparsity', type=float, default=0.); a('--head_sparsity', type=float, default=0.)
    a('--shrink_ratio', type=float, default=0.3, help='cost of the shrunk model as a fraction of the dense one')
    a('--bound', type=float, default=0.5, help='upper bound of a block\'s sparsity')
    a('--population', type=int, default=100)
    a('--rank-batches', type=int, default=1, help='training batches whose scores are summed for the ranking (the reference: 1)')
    a('--no-physical-shrink', dest='physical_shrink', action='store_false', default=True,
      help='evaluate each candidate MASKED at the dense cost, as the reference does (default: physically compacted, '
           'devit_amd.shrink.compact: the same function at the shrunk model\'s FLOPs)')
    a('--synthetic', type=int, default=0, metavar='STEPS', help='rank and evaluate on random on-device batches')
    return p


def load_weights(model, path, strict):
    ck = torch.load(path, map_location='cpu', weights_only=False)
    sd = ck['model'] if isinstance(ck, dict) and 'model' in ck else ck
    if not strict:                                   # shrink.py:305-310: a classifier of another class count is dropped
        own = model.state_dict()
        for k in ('head.weight', 'head.bias', 'head_dist.weight', 'head_dist.bias'):
            if k in sd and k in own and sd[k].shape != own[k].shape:
                print(f"Removing key {k} from pretrained checkpoint")
                del sd[k]
    model.load_state_dict(sd, strict=strict)


def main(args):
    if int(os.environ.get('WORLD_SIZE', '1')) > 1 or args.world_size > 1:
        raise SystemExit("shrink.py runs in a single process (the policy search evaluates its candidates one after the other on one GPU): "
                         "start it with plain `python shrink.py ...`, not under torch.distributed.run")
    check_input_size(args)
    args.distributed, args.rank, args.gpu = False, 0, 0
    device = torch.device(args.device)
    torch.manual_seed(args.seed)
    np.random.seed(args.seed)
    args.dataset = args.data_set                     # the name the dataset provider and distill_sub.py use
    args.dist_eval = False
    num_classes = NUM_CLASSES[args.data_set] // args.num_division
    train_loader, val_loader, num_classes = build_loaders(args, num_classes, device, provider="division")
    args.num_classes = num_classes

    model = devit_amd.create_model(args.model, pretrained=False, num_classes=num_classes, drop_rate=args.drop,
                                   drop_path_rate=args.drop_path, drop_block_rate=None, img_size=args.input_size)
    if args.finetune:
        load_weights(model, args.finetune, strict=False)
    if args.resume:
        load_weights(model, args.resume, strict=True)
    model.to(device)
    print(f"number of params: {sum(p.numel() for p in model.parameters() if p.requires_grad) / 1e6} M")

    # a ranking that is switched off leaves the units in their natural order (the reference dies on an undefined name there)
    geo = shrink_ops.model_geometry(model)
    neuron_rank = [np.arange(geo["emb"] * geo["mlp_ratio"]) for _ in range(geo["layer"])]
    head_rank = [np.arange(geo["head"]) for _ in range(geo["layer"])]
    if args.neuron_shrinking or args.head_shrinking:
        nr, hr = shrink_ops.rank_units(model, train_loader, device, batches=args.rank_batches)
        neuron_rank, head_rank = (nr if args.neuron_shrinking else neuron_rank), (hr if args.head_shrinking else head_rank)
    print(f"Finish ranking ({'neurons' if args.neuron_shrinking else 'natural neuron order'}, "
          f"{'heads' if args.head_shrinking else 'natural head order'}).")

    xp, yp = shrink_ops.search_policy(model, val_loader, neuron_rank, head_rank, args.shrink_ratio, args.population, 0, args.bound,
                                      device, args.seed, log=print, physical=args.physical_shrink)
    out = Path(args.output_dir) / f'{args.data_set}_div{args.num_division}' / f'{args.model}' / 'shrink'
    out.mkdir(parents=True, exist_ok=True)
    np.save(out / 'shrinked_policy.npy', xp)
    np.save(out / 'shrinked_accuracy.npy', yp)
    args.shrink_dir = str(out)
    print(f"Finish shrinking on sub-dataset{args.start_division}: best accuracy {float(yp.max()):.4f}, policies in {out}")
    return xp, yp


if __name__ == '__main__':
    parser = argparse.ArgumentParser('DeViT shrinking script (MI355X)', parents=[get_args_parser()])
    main(parser.parse_args())
