"""numpy restatement of the image-op layers (include/devit_hip.h, "Image ops": RandAugment's fifteen `inc1` operations and ColorJitter's three
enhancement steps on the S x S uint8 image), written from the header's statement and from PIL's sources (ImageOps.py, ImageEnhance.py, Blend.c,
Filter.c, Geometry.c), not from the kernels or from devit_amd/data.py: tests/test_randaug_model.py holds it to PIL (tests/golden/randaug_pil.npz,
and PIL live where it imports), tests/test_gpu_randaug.py holds the kernels to it, byte for byte.

A layer here is a dict: op (0 .. 14, timm's _RAND_INCREASING_TRANSFORMS order), filter (1 bilinear, 2 bicubic), factor (the blend ops), arg
(Posterize's bits, Solarize's threshold, SolarizeAdd's addend), matrix (six doubles, the affine family) and fill (three levels).

The second half restates the per-sample draws (timm 0.5.4's auto_augment.py / transforms_factory.py level formulas on a random.Random)."""
import math

import numpy as np

AUTOCONTRAST, EQUALIZE, INVERT, ROTATE, POSTERIZE, SOLARIZE, SOLARIZE_ADD, COLOR, CONTRAST, BRIGHTNESS, SHARPNESS, SHEAR_X, SHEAR_Y, \
    TRANSLATE_X, TRANSLATE_Y = range(15)
N_OPS, MAX_OPS = 15, 4
BILINEAR, BICUBIC = 1, 2
AFFINE_OPS = (ROTATE, SHEAR_X, SHEAR_Y, TRANSLATE_X, TRANSLATE_Y)
IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)
FILL = (124, 116, 104)          # tuple(min(255, round(255 * m)) for m in the ImageNet mean)


def layer(op, filter=BILINEAR, factor=1.0, arg=0, matrix=IDENTITY, fill=FILL):
    return dict(op=op, filter=filter, factor=float(factor), arg=int(arg), matrix=tuple(float(v) for v in matrix), fill=tuple(fill))


# ---- matrices (made on the host, in python floats = IEEE doubles) ----------------------------------------------------------------------------
def rotate_matrix(deg, S):
    """Image.rotate(deg) about the centre (S / 2, S / 2)"""
    t = -math.radians(deg % 360.0)
    m = [round(math.cos(t), 15), round(math.sin(t), 15), 0.0, round(-math.sin(t), 15), round(math.cos(t), 15), 0.0]
    cx = cy = S / 2.0
    m[2] = m[0] * (-cx) + m[1] * (-cy) + m[2] + cx
    m[5] = m[3] * (-cx) + m[4] * (-cy) + m[5] + cy
    return tuple(m)


def affine_matrix(op, v, S):
    """v: degrees (Rotate), the shear factor, or the translation in pixels"""
    if op == ROTATE:
        return rotate_matrix(v, S)
    return {SHEAR_X: (1.0, v, 0.0, 0.0, 1.0, 0.0), SHEAR_Y: (1.0, 0.0, 0.0, v, 1.0, 0.0), TRANSLATE_X: (1.0, 0.0, v, 0.0, 1.0, 0.0),
            TRANSLATE_Y: (1.0, 0.0, 0.0, 0.0, 1.0, v)}[op]


# ---- the ops -----------------------------------------------------------------------------------------------------------------------------------
def luma(img):
    i = img.astype(np.int64)
    return (19595 * i[..., 0] + 38470 * i[..., 1] + 7471 * i[..., 2] + 0x8000) >> 16


def blend(d, u, f, bug=None):
    """d + f (u - d) in fp32, one multiply and one add; truncated for 0 <= f <= 1, clipped and truncated outside"""
    if bug == "blend_double":
        r = d.astype(np.float64) + float(f) * (u.astype(np.float64) - d.astype(np.float64))
    elif bug == "blend_fma":
        r = (d.astype(np.float64) + np.float64(np.float32(f)) * (u.astype(np.float64) - d.astype(np.float64))).astype(np.float32)   # one rounding
    else:
        d32, u32 = d.astype(np.float32), u.astype(np.float32)
        r = d32 + np.float32(f) * (u32 - d32)
    if bug == "blend_round":
        r = np.floor(r.astype(np.float64) + 0.5)
    if 0.0 <= f <= 1.0:
        return r.astype(np.int64).astype(np.uint8)
    return np.where(r <= 0, 0, np.where(r >= 255, 255, r.astype(np.int64))).astype(np.uint8)


def smooth(img, bug=None):
    """ImageFilter.SMOOTH: fp32 accumulation of pixel * (k / 13) over the 3 x 3 window, + 0.5, clamp, truncate; the border is the image's"""
    S = img.shape[0]
    k = (np.array([1, 1, 1, 1, 5, 1, 1, 1, 1], np.float32) / np.float32(13.0)).astype(np.float32)
    src = np.pad(img, ((1, 1), (1, 1), (0, 0)), mode="edge").astype(np.float32) if bug == "smooth_border" else img.astype(np.float32)
    n = src.shape[0] - 2
    acc = np.zeros((n, n, 3), np.float32)
    for j in range(3):
        for i in range(3):
            acc = acc + src[j:j + n, i:i + n] * k[3 * j + i]
    acc = acc + np.float32(0.5)
    core = np.where(acc <= 0, 0, np.where(acc >= 255, 255, acc.astype(np.int64))).astype(np.uint8)
    if bug == "smooth_border":
        return core
    out = img.copy()
    out[1:S - 1, 1:S - 1] = core
    return out


def autocontrast_lut(h):
    nz = np.nonzero(h)[0]
    if len(nz) == 0 or nz[-1] <= nz[0]:
        return np.arange(256, dtype=np.uint8)
    lo, hi = int(nz[0]), int(nz[-1])
    scale = 255.0 / (hi - lo)
    off = -lo * scale
    return np.array([min(255, max(0, int(i * scale + off))) for i in range(256)], np.uint8)


def equalize_lut(h):
    nz = [int(v) for v in h if v]
    if len(nz) <= 1:
        return np.arange(256, dtype=np.uint8)
    step = (sum(nz) - nz[-1]) // 255
    if not step:
        return np.arange(256, dtype=np.uint8)
    lut, n = [], step // 2
    for i in range(256):
        lut.append(min(255, n // step))
        n += int(h[i])
    return np.array(lut, np.uint8)


def _taps(img, rows, cols):
    return img[rows, cols].astype(np.float64)


def affine(img, m, filt, fill, bug=None):
    """Image.transform(AFFINE, m, resample=filt, fillcolor=fill) on a square image: Geometry.c's affine_transform + bilinear / bicubic filter"""
    S = img.shape[0]
    a, b, c, d, e, f = (np.float64(v) for v in m)
    g = np.arange(S, dtype=np.float64) + 0.5
    X, Y = g[None, :], g[:, None]
    with np.errstate(all="ignore"):
        xin = a * X + b * Y + c
        yin = d * X + e * Y + f
        inside = (xin >= 0.0) & (xin < S) & (yin >= 0.0) & (yin < S)
    if bug == "fill_on_clamped_edges":             # the fill colour wherever a tap had to be clamped
        with np.errstate(all="ignore"):
            inside &= (xin >= 1.5) & (xin < S - 2.5) & (yin >= 1.5) & (yin < S - 2.5) if filt == BICUBIC else \
                (xin >= 0.5) & (xin < S - 1.5) & (yin >= 0.5) & (yin < S - 1.5)
    xin, yin = np.where(inside, xin, 0.5) - 0.5, np.where(inside, yin, 0.5) - 0.5
    x, y = np.floor(xin).astype(np.int64), np.floor(yin).astype(np.int64)
    dx, dy = (xin - x)[..., None], (yin - y)[..., None]
    cl = lambda v: np.clip(v, 0, S - 1)
    if filt == BICUBIC:
        def cubic(v1, v2, v3, v4, t):
            p1, p2, p3, p4 = v2, -v1 + v3, 2 * (v1 - v2) + v3 - v4, -v1 + v2 - v3 + v4
            return p1 + t * (p2 + t * (p3 + t * p4))
        rows = []
        for k in range(-1, 3):
            r = cubic(*[_taps(img, cl(y + k), cl(x + j)) for j in range(-1, 3)], dx)
            if k >= 0:
                ok = ((y + k >= 0) & (y + k < S))[..., None]
                r = np.where(ok, r, rows[-1])
            rows.append(r)
        v = cubic(*rows, dy)
        val = v.astype(np.int64) if bug == "cubic_no_clamp" else np.where(v <= 0.0, 0, np.where(v >= 255.0, 255, v.astype(np.int64)))
        val = val & 255
    else:
        def row(yy):
            p0, p1 = _taps(img, cl(yy), cl(x)), _taps(img, cl(yy), cl(x + 1))
            return p0 + (p1 - p0) * dx
        v1 = row(y)
        v2 = np.where(((y + 1 >= 0) & (y + 1 < S))[..., None], row(y + 1), v1)
        val = (v1 + (v2 - v1) * dy).astype(np.int64)
    return np.where(inside[..., None], val, np.asarray(fill, np.int64)[None, None, :]).astype(np.uint8)


def apply_op(img, L, bug=None):
    """uint8 [S][S][3], a layer -> uint8 [S][S][3]"""
    op, f, arg = L["op"], L["factor"], L["arg"]
    if op == INVERT:
        return (255 - img).astype(np.uint8)
    if op == POSTERIZE:
        return img & np.uint8(~((1 << (8 - arg)) - 1) & 255)
    if op == SOLARIZE:
        return np.where(img < arg, img, 255 - img).astype(np.uint8)
    if op == SOLARIZE_ADD:
        return np.where(img < 128, np.minimum(255, img.astype(np.int64) + arg), img).astype(np.uint8)
    if op in (AUTOCONTRAST, EQUALIZE):
        make = autocontrast_lut if op == AUTOCONTRAST else equalize_lut
        return np.stack([make(np.bincount(img[..., c].ravel(), minlength=256))[img[..., c]] for c in range(3)], axis=-1)
    if op == BRIGHTNESS:
        return blend(np.zeros_like(img), img, f, bug)
    if op == COLOR:
        return blend(np.repeat(luma(img)[..., None], 3, axis=-1), img, f, bug)
    if op == CONTRAST:
        total = int(luma(img).sum())
        mean = int(total / (img.shape[0] * img.shape[1]) + (0.0 if bug == "contrast_mean_floor" else 0.5))
        return blend(np.full_like(img, mean), img, f, bug)
    if op == SHARPNESS:
        return blend(smooth(img, bug), img, f, bug)
    if op in AFFINE_OPS:
        return affine(img, L["matrix"], L["filter"], L["fill"], bug)
    raise ValueError(f"op {op}")


def apply_layers(img, layers, bug=None):
    for L in (reversed(layers) if bug == "layers_reversed" else layers):
        img = apply_op(img, L, bug)
    return img


# ---- the draws -----------------------------------------------------------------------------------------------------------------------------------
def parse_rand(config):
    """'rand-m9-mstd0.5-inc1-n2' -> (m, n, mstd); only what the issue builds, the rest is the product's to refuse"""
    m, n, mstd = 10, 2, 0.0
    for part in config.split("-")[1:]:
        if part.startswith("mstd"):
            mstd = float(part[4:])
        elif part.startswith("inc"):
            assert part == "inc1"
        elif part.startswith("m"):
            m = int(part[1:])
        elif part.startswith("n"):
            n = int(part[1:])
    return m, n, mstd


def fill_colour(mean):
    return tuple(min(255, round(255 * v)) for v in mean)


def draw_rand_layers(rng, S, m, n, mstd, interpolation, fill=FILL):
    """the layers of one sample: n times (op, apply?, magnitude, sign, filter)"""
    layers = []
    for _ in range(n):
        op = rng.randrange(N_OPS)
        if rng.random() > 0.5:
            continue
        mag = float(m)
        if mstd > 0:
            mag = rng.uniform(0, mag) if mstd == float("inf") else rng.gauss(mag, mstd)
        lvl = min(10.0, max(0.0, mag)) / 10.0
        neg = lambda v: -v if rng.random() > 0.5 else v
        factor, arg, matrix, filt = 1.0, 0, IDENTITY, BILINEAR
        if op == ROTATE:
            matrix = rotate_matrix(neg(lvl * 30.0), S)
        elif op == POSTERIZE:
            arg = 4 - int(lvl * 4)
        elif op == SOLARIZE:
            arg = 256 - int(lvl * 256)
        elif op == SOLARIZE_ADD:
            arg = int(lvl * 110)
        elif op in (COLOR, CONTRAST, BRIGHTNESS, SHARPNESS):
            factor = 1.0 + neg(lvl * 0.9)
        elif op in (SHEAR_X, SHEAR_Y):
            matrix = affine_matrix(op, neg(lvl * 0.3), S)
        elif op in (TRANSLATE_X, TRANSLATE_Y):
            matrix = affine_matrix(op, neg(lvl * 0.45) * S, S)
        if op in AFFINE_OPS:
            filt = rng.choice((BILINEAR, BICUBIC)) if interpolation == "random" else {"bilinear": BILINEAR, "bicubic": BICUBIC}[interpolation]
        layers.append(layer(op, filt, factor, arg, matrix, fill))
    return layers


def draw_jitter_layers(rng, cj, fill=FILL):
    """ColorJitter(cj, cj, cj): a random order of (Brightness, Contrast, Color), then the three factors in that argument order"""
    order = [0, 1, 2]
    rng.shuffle(order)
    factors = [rng.uniform(max(0.0, 1.0 - cj), 1.0 + cj) for _ in range(3)]
    return [layer((BRIGHTNESS, CONTRAST, COLOR)[k], factor=factors[k], fill=fill) for k in order]


# ---- the golden file -----------------------------------------------------------------------------------------------------------------------------
def golden_cases(g):
    """[(source uint8 [S][S][3], [layers], PIL's result uint8 [S][S][3])] of tests/golden/randaug_pil.npz (already loaded)"""
    out, at = [], 0
    for src, index, first, count in g["cases"]:
        img = g[str(g["sources"][src])][index]
        layers = [layer(int(r[0]), int(r[1]), float(f[0]), int(r[2]), tuple(f[1:7]), tuple(int(v) for v in r[3:6]))
                  for r, f in zip(g["layers_i"][first:first + count], g["layers_f"][first:first + count])]
        n = img.size
        out.append((img, layers, g["pixels"][at:at + n].reshape(img.shape)))
        at += n
    return out
