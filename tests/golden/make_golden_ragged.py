#!/usr/bin/env python3
"""Writes tests/golden/augment_ragged_pil.npz: what PIL makes of crop-then-resize on deterministic uint8 sources of DIFFERING sizes, for the
cases the packed-set kernels are held to (include/devit_hip.h, "Packed sets"): crops that need 13 .. 59 taps beside ones the 12-tap kernel
serves.  Imports PIL and numpy only (and the numpy model under tests/, to assert that it equals PIL on every case written); the tests read
the file and never import PIL.  The layout is make_golden_augment.py's:

    sources   names of the source arrays in the file, each [1][H][W][3]
    cases     int32 [n][13]: source, index in it (0), y0, x0, h, w, Rh, Rw, oy, ox, filter (0 none, 1 bilinear, 2 bicubic), S, offset into pixels
    pixels    uint8, the cases' windows [S][S][3] one behind the other

Every box has h <= 16 w: PIL makes the vertical pass first for boxes about 107 or more times as tall as wide, the definition is horizontal
first for every box.  A case on which the model and PIL differ is dropped and reported, never tolerated."""
import os
import sys

import numpy as np
from PIL import Image

from make_golden_augment import BICUBIC, BILINEAR, NONE, PIL_FILTER, eval_geometry

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _augment_model as M      # noqa: E402
import _ragged_model as RM      # noqa: E402

SIZES = [(20, 28), (33, 35), (200, 61), (61, 330), (150, 170), (40, 700), (146, 145)]      # H x W


def sources():
    rng = np.random.RandomState(20240611)

    def make(n, H, W):      # make_golden_augment.py's generator
        y, x = np.mgrid[0:H, 0:W]
        out = []
        for i in range(n):
            base = 128 + 100 * np.sin((y * (i + 2) + x * 3) / 7.0)[:, :, None] * np.array([1.0, -0.7, 0.4])
            img = np.clip(base + rng.randint(-40, 41, (H, W, 3)), 0, 255)
            img[H // 4:H // 2, W // 3:W // 2] = 255 * (i % 2)
            img[0, :] = 255 - 255 * (i % 2)
            out.append(img.astype(np.uint8))
        return np.stack(out)
    return {f"src{H}x{W}": make(1, H, W) for H, W in SIZES}


def cases():
    out = []

    def add(hw, box, S, filt, virt=None):
        assert box[2] <= 16 * box[3], box
        out.append((f"src{hw[0]}x{hw[1]}", 0, *box, *(virt or (S, S, 0, 0)), filt, S))
    rng = np.random.RandomState(11)
    # every source whole at 48, both filters: 146 x 145 bicubic is the boundary between the kernels (13 taps vertically, 12 horizontally),
    # 61 x 330 is narrow on one axis with 28 taps on the other
    for H, W in SIZES:
        for filt in (BILINEAR, BICUBIC):
            add((H, W), (0, 0, H, W), 48, filt)
    # boxes on each edge of two sources, the degenerate boxes
    for (H, W), filt in (((150, 170), BICUBIC), ((61, 330), BILINEAR)):
        for box in ((0, 7, H // 2, W // 2), (H - H // 2, 7, H // 2, W // 2), (5, 0, H // 2, W // 3), (5, W - W // 3, H // 2, W // 3)):
            add((H, W), box, 48, filt)
    add((40, 700), (3, 690, 1, 5), 48, BICUBIC)
    add((200, 61), (190, 60, 5, 1), 48, BILINEAR)
    # random boxes
    for k in range(8):
        H, W = SIZES[2 + k % 5]
        h = int(rng.randint(3, H + 1))
        w = int(rng.randint(max(3, (h + 15) // 16), W + 1))
        add((H, W), (int(rng.randint(0, H - h + 1)), int(rng.randint(0, W - w + 1)), h, w), 48, (BILINEAR, BICUBIC)[k % 2])
    # the eval geometry of every source
    for H, W in SIZES:
        add((H, W), (0, 0, H, W), 48, BICUBIC, eval_geometry(H, W, 48))
    # at 32 with a filter: 42 taps; 25 taps vertically, more than the narrow kernel's 24 intermediate rows
    add((61, 330), (0, 0, 61, 330), 32, BICUBIC)
    add((200, 61), (0, 0, 200, 61), 32, BICUBIC)
    # at 224: 13 taps, whole-row stores, the last band; the eval geometry
    add((40, 700), (0, 0, 40, 700), 224, BICUBIC)
    add((61, 330), (0, 0, 61, 330), 224, BICUBIC, eval_geometry(61, 330, 224))
    # the padded crop RandomCrop(32, padding=4) on 33 x 35 at its corner offsets
    for y0, x0 in ((-4, -4), (-4, 7), (5, -4), (5, 7)):
        add((33, 35), (y0, x0, 32, 32), 32, NONE)
    return out


def main():
    src = sources()
    names = sorted(src)
    rows, pixels, offset, dropped = [], [], 0, []
    for name, index, y0, x0, h, w, Rh, Rw, oy, ox, filt, S in cases():
        im = Image.fromarray(src[name][index]).crop((x0, y0, x0 + w, y0 + h))
        if filt != NONE:
            im = im.resize((Rw, Rh), PIL_FILTER[filt]).crop((ox, oy, ox + S, oy + S))
        px = np.asarray(im, dtype=np.uint8)
        assert px.shape == (S, S, 3), px.shape
        if not np.array_equal(RM.resample(src[name][index], M.row(y0, x0, h, w, S, Rh, Rw, oy, ox, filt), S), px):
            dropped.append((name, y0, x0, h, w, Rh, Rw, filt, S))
            continue
        rows.append((names.index(name), index, y0, x0, h, w, Rh, Rw, oy, ox, filt, S, offset))
        pixels.append(px.reshape(-1))
        offset += px.size
    path = os.path.join(HERE, "augment_ragged_pil.npz")
    np.savez_compressed(path, sources=np.array(names), cases=np.array(rows, dtype=np.int32), pixels=np.concatenate(pixels), **src)
    print(path, len(rows), "cases,", os.path.getsize(path), "bytes; dropped (the model differs from PIL):", dropped)
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
