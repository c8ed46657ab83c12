#!/usr/bin/env python3
"""Generate tests/golden/ensemble_kldiv.npz by running the REFERENCE's own modules on CPU fp32, through the shims of make_golden.py.

Runs only in the build container (needs the reference tree; never on the GPU box); nothing of the reference is copied, OUTPUTS only.

  ensemble_kldiv.npz   the ensemble step of ensemble.npz (make_golden.make_ensemble: bs 4, MultiViT of 4 x dedeit, EnsMLP, DeiT-B teacher,
                       hard distillation, the same deterministic weights, images and targets) with the reference's own
                       EnsLoss(loss_type='kldiv') (utils/losses.py:192-193): token_loss, cls_loss and the four gradient slices of ensemble.npz

Usage:  python tests/golden/make_golden_kldiv.py
"""
import functools
import os
import sys

import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as MG  # noqa: E402  (the shims, save(), ens_state())
from oracle.detgen import det_array, det_labels  # noqa: E402
from oracle import devit_oracle as O  # noqa: E402


def main():
    torch.set_num_threads(8)
    torch.manual_seed(0)
    MG.install_shims()
    import models.de_vit as de_vit          # noqa: E402  (reference)
    import models.ensemble_models as em     # noqa: E402  (reference)
    import utils.losses as ref_losses       # noqa: E402  (reference)

    gs, gt = O.GEOMETRY["dedeit"], O.GEOMETRY["deit_base_distilled_patch16_224"]
    multi = em.MultiViT(model="dedeit", drop=0, drop_path=0.0, num_classes_list=[25] * 4, num_div=4)
    ens = em.EnsMLP(model="dedeit", num_class=100, sub_size=384, num_classes_list=[25] * 4, teacher_size=768)
    sd = multi.state_dict()
    keys = list(sd.keys())
    for i in range(4):                            # positional copy, as make_golden.make_ensemble
        sub = O.make_state(gs, 25, f"E{i}")
        src = list(sub.keys())
        for j in range(len(src) - 4):
            sd[keys[i * (len(src) - 4) + j]] = sub[src[j]]
    multi.load_state_dict(sd)
    ens.load_state_dict(MG.ens_state())
    teacher = de_vit.VisionTransformer(patch_size=16, embed_dim=768, depth=12, num_heads=12, mlp_ratio=4, qkv_bias=True,
                                       norm_layer=functools.partial(nn.LayerNorm, eps=1e-6), distilled=True, num_classes=100)
    teacher.load_state_dict(O.make_state(gt, 100, "T100"))
    teacher.eval()
    img = torch.from_numpy(det_array("img4", (4, 3, 224, 224)))
    multi.train(); ens.train()
    tokens, logits = ens(multi(img), True)
    y = det_labels("ens_y", 4, 100)
    soft = torch.full((4, 100), 0.1 / 100).scatter_(1, torch.from_numpy(y)[:, None], 0.9 + 0.1 / 100)
    crit = ref_losses.EnsLoss(sys.modules["timm.loss"].SoftTargetCrossEntropy(), teacher, "dedeit", "hard", 0.5, 1.0, loss_type="kldiv")
    token_loss, cls_loss = crit(img, (tokens, logits), soft)
    (token_loss + cls_loss).backward()
    MG.save("ensemble_kldiv", token_loss=token_loss, cls_loss=cls_loss, soft_targets=soft,
            g_cls_mlp_w_rows=ens.cls_mlp.weight.grad[::48], g_dist_cls_w=ens.dist_classifier.weight.grad[::10],
            g_b2_fc1_rows=multi.backbones[2].blocks[3].mlp.fc1.weight.grad[::96],
            g_b0_pos=multi.backbones[0].pos_embed.grad[0, ::16])


if __name__ == "__main__":
    main()
