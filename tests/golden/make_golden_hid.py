#!/usr/bin/env python3
"""Generate tests/golden/hid_relation.npz by running the REFERENCE's own cal_hid_relation_loss (utils/losses.py:295-304) on CPU fp32, through the
shims of make_golden.py.

Runs only in the build container (needs the reference tree; never on the GPU box); nothing of the reference is copied, OUTPUTS only.

  hid_relation.npz   two layer pairs, B = 2, N = 7, student width 64, teacher width 128; the inputs are oracle.detgen arrays
                     (tests/_hid_model.golden_inputs regenerates them): the loss and the gradient of each student tensor

Usage:  python tests/golden/make_golden_hid.py
"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as MG  # noqa: E402  (the shims, save())
import _hid_model as HM  # noqa: E402


def main():
    torch.set_num_threads(8)
    MG.install_shims()
    import utils.losses as ref_losses       # noqa: E402  (reference)

    stu, tea = HM.golden_inputs()
    stu = [s.clone().requires_grad_(True) for s in stu]
    loss = ref_losses.cal_hid_relation_loss(stu, tea)
    loss.backward()
    MG.save("hid_relation", loss=loss, **{f"grad_s{i}": s.grad for i, s in enumerate(stu)})


if __name__ == "__main__":
    main()
