#!/usr/bin/env python3
"""Writes tests/golden/augment_pil.npz: what PIL makes of crop-then-resize on deterministic uint8 sources, for the cases the input-augmentation
kernels are held to (include/devit_hip.h, "Input augmentation").  Imports PIL and numpy only; the tests read the file and never import PIL.

    sources   names of the source arrays in the file: src32 [4][32][32][3], src2028 [2][20][28][3], src48 [2][48][48][3]
    cases     int32 [n][13]: source, index in it, y0, x0, h, w, Rh, Rw, oy, ox, filter (0 none, 1 bilinear, 2 bicubic), S, offset into pixels
    pixels    uint8, the cases' windows [S][S][3] one behind the other:
              Image.fromarray(src).crop((x0, y0, x0 + w, y0 + h)).resize((Rw, Rh), filter).crop((ox, oy, ox + S, oy + S)); filter 0: the first crop alone
"""
import os

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
NONE, BILINEAR, BICUBIC = 0, 1, 2
PIL_FILTER = {BILINEAR: Image.BILINEAR, BICUBIC: Image.BICUBIC}


def sources():
    rng = np.random.RandomState(20240611)

    def make(n, H, W):
        # a smooth ramp plus noise plus a few saturated blocks: overshoot of the cubic has something to clip at both ends
        y, x = np.mgrid[0:H, 0:W]
        out = []
        for i in range(n):
            base = 128 + 100 * np.sin((y * (i + 2) + x * 3) / 7.0)[:, :, None] * np.array([1.0, -0.7, 0.4])
            img = np.clip(base + rng.randint(-40, 41, (H, W, 3)), 0, 255)
            img[H // 4:H // 2, W // 3:W // 2] = 255 * (i % 2)
            img[0, :] = 255 - 255 * (i % 2)
            out.append(img.astype(np.uint8))
        return np.stack(out)
    return {"src32": make(4, 32, 32), "src2028": make(2, 20, 28), "src48": make(2, 48, 48)}


def eval_geometry(H0, W0, S):
    """torchvision Resize(int(256 / 224 * S)) + CenterCrop(S): (Rh, Rw, oy, ox)"""
    R = int(256 / 224 * S)
    if H0 <= W0:
        Rh, Rw = R, int(R * W0 / H0)
    else:
        Rh, Rw = int(R * H0 / W0), R
    return Rh, Rw, int(round((Rh - S) / 2.)), int(round((Rw - S) / 2.))


def cases():
    out = []

    def add(src, index, box, S, filt, virt=None):
        H0, W0 = {"src32": (32, 32), "src2028": (20, 28), "src48": (48, 48)}[src]
        out.append((src, index, *box, *(virt or (S, S, 0, 0)), filt, S))
    rng = np.random.RandomState(7)
    # 32 x 32 sources -> 48: the degenerate boxes, the whole image, boxes on each edge, random ones; both filters
    boxes32 = [(0, 0, 1, 5), (7, 30, 5, 1), (10, 11, 3, 3), (0, 0, 32, 32), (0, 5, 10, 12), (22, 5, 10, 12), (5, 0, 12, 10), (5, 22, 12, 10),
               (31, 31, 1, 1), (0, 0, 32, 3)]
    for _ in range(4):
        h, w = rng.randint(3, 33, 2)
        boxes32.append((int(rng.randint(0, 33 - h)), int(rng.randint(0, 33 - w)), int(h), int(w)))
    for i, box in enumerate(boxes32):
        for filt in (BILINEAR, BICUBIC):
            add("src32", i % 4, box, 48, filt)
    # ... -> 32 with a filter (1:1 on the whole image is the identity; smaller boxes are not)
    for box, filt in (((0, 0, 32, 32), BICUBIC), ((3, 1, 27, 30), BILINEAR), ((8, 9, 16, 7), BICUBIC)):
        add("src32", 1, box, 32, filt)
    # the non-square source
    for box, S, filt in (((0, 0, 20, 28), 48, BICUBIC), ((2, 3, 17, 9), 48, BILINEAR), ((0, 19, 20, 9), 32, BICUBIC), ((11, 0, 9, 28), 32, BILINEAR)):
        add("src2028", len(out) % 2, box, S, filt)
    # down-scaling: 48 x 48 -> 32, both filters, and a non-square box that scales down on one axis and up on the other
    for box, filt in (((0, 0, 48, 48), BILINEAR), ((0, 0, 48, 48), BICUBIC), ((0, 4, 48, 20), BICUBIC), ((5, 0, 40, 48), BILINEAR)):
        add("src48", len(out) % 2, box, 32, filt)
    # the eval geometry: Resize(int(256 / 224 * S)) + CenterCrop(S), bicubic, at 48 (square and not) and at 224
    add("src32", 2, (0, 0, 32, 32), 48, BICUBIC, eval_geometry(32, 32, 48))
    add("src2028", 0, (0, 0, 20, 28), 48, BICUBIC, eval_geometry(20, 28, 48))
    add("src32", 3, (0, 0, 32, 32), 224, BICUBIC, eval_geometry(32, 32, 224))
    # a train crop at 224: whole-row stores and the last band
    add("src32", 0, (4, 6, 20, 17), 224, BILINEAR)
    # the padded crop RandomCrop(32, padding=4) at its four corner offsets and in the middle
    for y0, x0 in ((-4, -4), (-4, 4), (4, -4), (4, 4), (0, 0), (-1, 3)):
        add("src32", len(out) % 4, (y0, x0, 32, 32), 32, NONE)
    return out


def main():
    src = sources()
    names = sorted(src)
    rows, pixels, offset = [], [], 0
    for name, index, y0, x0, h, w, Rh, Rw, oy, ox, filt, S in cases():
        im = Image.fromarray(src[name][index]).crop((x0, y0, x0 + w, y0 + h))
        if filt != NONE:
            im = im.resize((Rw, Rh), PIL_FILTER[filt]).crop((ox, oy, ox + S, oy + S))
        px = np.asarray(im, dtype=np.uint8)
        assert px.shape == (S, S, 3), px.shape
        rows.append((names.index(name), index, y0, x0, h, w, Rh, Rw, oy, ox, filt, S, offset))
        pixels.append(px.reshape(-1))
        offset += px.size
    path = os.path.join(HERE, "augment_pil.npz")
    np.savez_compressed(path, sources=np.array(names), cases=np.array(rows, dtype=np.int32), pixels=np.concatenate(pixels), **src)
    print(path, len(rows), "cases,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
