#!/usr/bin/env python3
"""Generate tests/golden/imgsize_*.npz by running the REFERENCE's own code on CPU fp32, through the shims of make_golden.py.

Runs only in the build container (needs the reference tree; never on the GPU box); nothing of the reference is copied, OUTPUTS only.

  imgsize_dedeit48.npz   the reference's `dedeit` built with img_size=48 (3 x 3 patches + 2 tokens = 11 rows), the deterministic weights
                         of tests/_imgsize_model.make_state(..., "S", 48), 2 images: logits, top-1, train-mode outputs, q/k/v of block 5,
                         the last tokens (q/k/v: two heads; the last encoder output: every 8th column) -- what pins the size-general
                         CPU helper (tests/test_imgsize_host.py)
  imgsize_resize.npz     the reference's resize_pos_embed (models/de_vit.py:452-473) on the deterministic [1, 198, 64] table of
                         _imgsize_model.pos_embed_input(), 14 x 14 -> 7 x 7 and 14 x 14 -> 3 x 3, two token rows kept

Usage:  python tests/golden/make_golden_imgsize.py
"""
import contextlib
import io
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as MG  # noqa: E402  (the shims, save(), load_into())
import _imgsize_model as IM  # noqa: E402
from oracle.detgen import det_array  # noqa: E402
from oracle import devit_oracle as O  # noqa: E402


def main():
    torch.set_num_threads(8)
    torch.manual_seed(0)
    _, create_model, _ = MG.install_shims()
    import models.de_vit as de_vit          # noqa: E402  (reference)

    C, S = 25, 48
    gs = O.GEOMETRY["dedeit"]
    model = create_model("dedeit", pretrained=False, num_classes=C, drop_rate=0.0, drop_path_rate=0.0, drop_block_rate=None, img_size=S)
    MG.load_into(model, IM.make_state(gs, C, "S", S))
    img = torch.from_numpy(det_array("imgsize/img48", (2, 3, S, S)))
    model.eval()
    with torch.no_grad():
        logits = model(img)
        d = model(img, distill_token=True, output_qkv=True, output_att=True, output_emb=True, output_encoders=True)
    assert torch.equal(d["output"], logits)
    q, k, v = d["qkv"][5]
    model.train()
    with torch.no_grad():
        tr = model(img)
    MG.save("imgsize_dedeit48", logits=logits, top1=logits.argmax(1), train_cls=tr[0], train_dist=tr[1], q5=q[:, :2], k5=k[:, :2],
            v5=v[:, :2], enc_last=d["encoder"][-1][:, :, ::8], last_cls=d["last_tokens"][0],
            last_dist=d["last_tokens"][1], n_keys=len(model.state_dict()), pos_shape=list(model.pos_embed.shape))

    pe = IM.pos_embed_input()
    with contextlib.redirect_stdout(io.StringIO()):        # (the reference prints the shapes)
        to7 = de_vit.resize_pos_embed(pe, torch.zeros(1, 51, 64), 2, (7, 7))
        to3 = de_vit.resize_pos_embed(pe, torch.zeros(1, 11, 64), 2, (3, 3))
    MG.save("imgsize_resize", to7=to7, to3=to3)
    print("done")


if __name__ == "__main__":
    main()
