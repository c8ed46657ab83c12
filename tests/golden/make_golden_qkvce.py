#!/usr/bin/env python3
"""Generate tests/golden/qkvce.npz by running the REFERENCE's own cal_qkv_loss, cal_qkv_loss2 and soft_cross_entropy (utils/losses.py:37-41, 247-292)
on CPU fp32, through the shims of make_golden.py.

Runs only in the build container (needs the reference tree; never on the GPU box); nothing of the reference is copied, OUTPUTS only.

  qkvce.npz   inputs are oracle.detgen arrays (tests/_qkvce_model.golden_inputs / golden_ce_inputs regenerate them): B = 2, N = 5, student 2 heads,
              teacher 3 heads, head width 64 -- the smallest shape where the rows of `.view(B, N, H * 64)` straddle heads for both models.
              self1 / cross1: a single-pair list; self2 / cross2: the two-pair list; per case the loss and the gradient of every student tensor.
              ce0 / ce1: soft_cross_entropy on [3, 7] and [2, 5, 5]: the loss and the gradient of `predicts`.

Usage:  python tests/golden/make_golden_qkvce.py
"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as MG  # noqa: E402  (the shims, save())
import _qkvce_model as QM  # noqa: E402


def main():
    torch.set_num_threads(8)
    MG.install_shims()
    import utils.losses as ref_losses       # noqa: E402  (reference)

    out = {}
    stu, tea = QM.golden_inputs()
    for name, fn in (("self", ref_losses.cal_qkv_loss), ("cross", ref_losses.cal_qkv_loss2)):
        for pairs in (1, 2):
            s = [tuple(x.clone().requires_grad_(True) for x in qkv) for qkv in stu[:pairs]]
            loss = fn(s, tea[:pairs])
            loss.backward()
            out[f"{name}{pairs}_loss"] = loss
            for li, qkv in enumerate(s):
                for c, x in zip("qkv", qkv):
                    out[f"{name}{pairs}_grad_{li}{c}"] = x.grad
    for i, (p, t) in enumerate(QM.golden_ce_inputs()):
        p = p.clone().requires_grad_(True)
        loss = ref_losses.soft_cross_entropy(p, t)
        loss.backward()
        out[f"ce{i}_loss"], out[f"ce{i}_grad"] = loss, p.grad
    MG.save("qkvce", **out)


if __name__ == "__main__":
    main()
