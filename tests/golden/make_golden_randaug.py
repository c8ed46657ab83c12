#!/usr/bin/env python3
"""Writes tests/golden/randaug_pil.npz: what PIL makes of RandAugment's fifteen `inc1` operations and of ColorJitter's three enhancement steps, called
as timm 0.5.4's auto_augment.py calls them, on deterministic 32 x 32 and 48 x 48 uint8 sources (include/devit_hip.h, "Image ops").  Imports PIL and
numpy only; the tests read the file and never need PIL for it.

    sources    names of the source arrays: src32 [6][32][32][3] (four ramp + noise + saturated-block images, one with a constant channel, one of two
               levels), src48 [2][48][48][3]
    cases      int32 [n][4]: source, index in it, first layer, number of layers
    layers_i   int32 [m][6]: op (timm's _RAND_INCREASING_TRANSFORMS order), filter (1 bilinear, 2 bicubic), integer argument, fill r, g, b
    layers_f   float64 [m][8]: blend factor, the affine matrix a .. f, and the value the matrix was made from (degrees, shear, pixels)
    pixels     uint8, the cases' results [S][S][3] one behind the other
"""
import math
import os

import numpy as np
from PIL import Image, ImageEnhance, ImageOps

HERE = os.path.dirname(os.path.abspath(__file__))
AUTOCONTRAST, EQUALIZE, INVERT, ROTATE, POSTERIZE, SOLARIZE, SOLARIZE_ADD, COLOR, CONTRAST, BRIGHTNESS, SHARPNESS, SHEAR_X, SHEAR_Y, \
    TRANSLATE_X, TRANSLATE_Y = range(15)
BILINEAR, BICUBIC = 1, 2
PIL_FILTER = {BILINEAR: Image.BILINEAR, BICUBIC: Image.BICUBIC}
FILL = (124, 116, 104)
IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)


def sources():
    rng = np.random.RandomState(20240611)

    def make(n, S):
        y, x = np.mgrid[0:S, 0:S]
        out = []
        for i in range(n):
            base = 128 + 100 * np.sin((y * (i + 2) + x * 3) / 7.0)[:, :, None] * np.array([1.0, -0.7, 0.4])
            img = np.clip(base + rng.randint(-40, 41, (S, S, 3)), 0, 255)
            img[S // 4:S // 2, S // 3:S // 2] = 255 * (i % 2)
            img[0, :] = 255 - 255 * (i % 2)
            out.append(img.astype(np.uint8))
        return out
    s32 = make(4, 32)
    const = s32[0].copy()
    const[:, :, 1] = 77                                  # a constant channel: one histogram bin
    two = np.where(rng.randint(0, 4, (32, 32, 3)) == 0, 40, 200).astype(np.uint8)
    two[:, :, 2] = np.where(np.arange(32)[None, :] == 5, 9, 250)      # 32 pixels of one level, 992 of the other: Equalize's step is 0
    return {"src32": np.stack(s32 + [const, two]), "src48": np.stack(make(2, 48))}


def rotate_matrix(deg, S):
    t = -math.radians(deg % 360.0)
    m = [round(math.cos(t), 15), round(math.sin(t), 15), 0.0, round(-math.sin(t), 15), round(math.cos(t), 15), 0.0]
    c = S / 2.0
    m[2] = m[0] * (-c) + m[1] * (-c) + m[2] + c
    m[5] = m[3] * (-c) + m[4] * (-c) + m[5] + c
    return tuple(m)


def L(op, value=0.0, filt=BILINEAR):
    """(op, filter, integer argument, factor, value)"""
    if op in (POSTERIZE, SOLARIZE, SOLARIZE_ADD):
        return (op, filt, int(value), 1.0, 0.0)
    if op in (COLOR, CONTRAST, BRIGHTNESS, SHARPNESS):
        return (op, filt, 0, float(value), 0.0)
    return (op, filt, 0, 1.0, float(value))


def matrix_of(op, v, S):
    return {ROTATE: rotate_matrix(v, S), SHEAR_X: (1.0, v, 0.0, 0.0, 1.0, 0.0), SHEAR_Y: (1.0, 0.0, 0.0, v, 1.0, 0.0),
            TRANSLATE_X: (1.0, 0.0, v, 0.0, 1.0, 0.0), TRANSLATE_Y: (1.0, 0.0, 0.0, 0.0, 1.0, v)}.get(op, IDENTITY)


def pil_op(img, op, filt, arg, factor, value):
    """timm 0.5.4 auto_augment.py, op by op"""
    kw = dict(resample=PIL_FILTER[filt], fillcolor=FILL)
    if op == AUTOCONTRAST:
        return ImageOps.autocontrast(img)
    if op == EQUALIZE:
        return ImageOps.equalize(img)
    if op == INVERT:
        return ImageOps.invert(img)
    if op == ROTATE:
        return img.rotate(value, **kw)
    if op == POSTERIZE:
        return ImageOps.posterize(img, arg)
    if op == SOLARIZE:
        return ImageOps.solarize(img, arg)
    if op == SOLARIZE_ADD:
        lut = [min(255, i + arg) if i < 128 else i for i in range(256)]
        return img.point(lut + lut + lut)
    if op in (COLOR, CONTRAST, BRIGHTNESS, SHARPNESS):
        return {COLOR: ImageEnhance.Color, CONTRAST: ImageEnhance.Contrast, BRIGHTNESS: ImageEnhance.Brightness,
                SHARPNESS: ImageEnhance.Sharpness}[op](img).enhance(factor)
    return img.transform(img.size, Image.AFFINE, matrix_of(op, value, img.size[0]), **kw)


def cases():
    out = []

    def add(src, index, *layers):
        out.append((src, index, list(layers)))
    k = 0
    for op in (AUTOCONTRAST, EQUALIZE, INVERT):
        for src, index in (("src32", 0), ("src32", 3), ("src32", 4), ("src32", 5), ("src48", 1)):
            add(src, index, L(op))
    for bits in (0, 1, 2, 3, 4):
        add("src32", bits % 4, L(POSTERIZE, bits))
    for thresh in (0, 1, 26, 128, 255, 256):
        add("src32", thresh % 4, L(SOLARIZE, thresh))
    for a in (0, 1, 55, 99, 110):
        add("src32", a % 4, L(SOLARIZE_ADD, a))
    for op in (COLOR, CONTRAST, BRIGHTNESS, SHARPNESS):
        for f in (0.1, 0.55, 1.0, 1.45, 1.9):
            for src, index in (("src32", k % 6), ("src48", k % 2)):
                add(src, index, L(op, f))
            k += 1
    for filt in (BILINEAR, BICUBIC):
        for deg in (0.0, 30.0, -30.0, 13.5, -7.25):
            add("src32", k % 4, L(ROTATE, deg, filt))
            k += 1
        add("src48", 0, L(ROTATE, 27.0, filt))
        for op in (SHEAR_X, SHEAR_Y):
            for v in (0.3, -0.3, 0.11, 0.0):
                add("src32", k % 4, L(op, v, filt))
                k += 1
            add("src48", 1, L(op, -0.27, filt))
        for op in (TRANSLATE_X, TRANSLATE_Y):
            for frac in (0.45, -0.45, 0.2, -0.013, 1.0, -1.5, 0.0):          # 1.0 and -1.5: the whole image leaves
                add("src32", k % 4, L(op, frac * 32, filt))
                k += 1
            add("src48", 0, L(op, 0.333 * 48, filt))
    # chains: two and four layers, and ColorJitter orders
    add("src32", 1, L(EQUALIZE), L(ROTATE, 22.0, BICUBIC))
    add("src32", 2, L(SHEAR_X, 0.25, BILINEAR), L(SHARPNESS, 1.8))
    add("src48", 0, L(COLOR, 1.7), L(AUTOCONTRAST))
    add("src32", 3, L(TRANSLATE_Y, -9.0, BICUBIC), L(CONTRAST, 0.3), L(POSTERIZE, 2), L(SHEAR_Y, -0.2, BILINEAR))
    add("src48", 1, L(ROTATE, -17.0, BICUBIC), L(EQUALIZE), L(SHARPNESS, 0.2), L(SOLARIZE, 100))
    add("src32", 0, L(BRIGHTNESS, 0.7), L(CONTRAST, 1.3), L(COLOR, 0.65))
    add("src32", 4, L(COLOR, 1.38), L(BRIGHTNESS, 1.21), L(CONTRAST, 0.62))
    add("src48", 1, L(CONTRAST, 1.05), L(COLOR, 0.9), L(BRIGHTNESS, 1.4))
    return out


def main():
    src = sources()
    names = sorted(src)
    rows, li, lf, pixels = [], [], [], []
    for name, index, layers in cases():
        img = Image.fromarray(src[name][index])
        S = img.size[0]
        rows.append((names.index(name), index, len(li), len(layers)))
        for op, filt, arg, factor, value in layers:
            img = pil_op(img, op, filt, arg, factor, value)
            li.append((op, filt, arg, *FILL))
            lf.append((factor, *matrix_of(op, value, S), value))
        px = np.asarray(img, dtype=np.uint8)
        assert px.shape == (S, S, 3), px.shape
        pixels.append(px.reshape(-1))
    path = os.path.join(HERE, "randaug_pil.npz")
    np.savez_compressed(path, sources=np.array(names), cases=np.array(rows, dtype=np.int32), layers_i=np.array(li, dtype=np.int32),
                        layers_f=np.array(lf, dtype=np.float64), pixels=np.concatenate(pixels), **src)
    print(path, len(rows), "cases,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
