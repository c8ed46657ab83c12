"""numpy restatement of the packed-set form of the input-augmentation stage (include/devit_hip.h, "Packed sets"), written from the header's
statement: tests/_augment_model.py's resampling with its 12-tap cap lifted, the image found through a directory of (offset, H, W) into one
byte arena, and the closed-form tap bound that decides which of the two kernels serves a sample.  tests/test_ragged_model.py holds it to PIL
(tests/golden/augment_ragged_pil.npz, and PIL live where it imports), tests/test_gpu_ragged.py holds the kernels to it.

The definition never cuts a weight: the bound is never below the exact tap count, so the narrow kernel (12 weights) only ever gets samples
that fit it.  The planted bugs say what a kernel would compute if that, or the directory lookup, went wrong."""
import math

import numpy as np

import _augment_model as M

TAPS, TAPS_MAX, ALIGN = 12, 128, 16
BUGS = ("neighbour_base", "wrong_pitch", "weights_cut", "kind_wrong_axis", "no_intermediate")


# ---- the closed-form bound ---------------------------------------------------------------------------------------------------------------------
def taps_bound(length, R, filt):
    """min(floor(2 * support) + 1, length), support = (1 | 2) * max(length / R, 1); 1 at unit scale"""
    if filt == M.NONE:
        return 1
    support = (2.0 if filt == M.BICUBIC else 1.0) * max(float(length) / float(R), 1.0)
    return min(int(math.floor(2.0 * support)) + 1, length)


def is_wide(r, bug=None):
    if bug == "kind_wrong_axis":      # both axes judged by the vertical one
        return taps_bound(r["h"], r["Rh"], r["filter"]) > TAPS
    return max(taps_bound(r["h"], r["Rh"], r["filter"]), taps_bound(r["w"], r["Rw"], r["filter"])) > TAPS


def max_taps(rows):
    return max(max(taps_bound(r["h"], r["Rh"], r["filter"]), taps_bound(r["w"], r["Rw"], r["filter"])) for r in rows)


# ---- the packed set ----------------------------------------------------------------------------------------------------------------------------
def pack(images):
    """[uint8 [H][W][3]] -> (arena uint8 [bytes], [(offset, H, W)]): HWC, one behind the other, each at a multiple of 16"""
    entries, at = [], 0
    for a in images:
        entries.append((at, a.shape[0], a.shape[1]))
        at += (a.size + ALIGN - 1) // ALIGN * ALIGN
    arena = np.zeros(at, dtype=np.uint8)
    for (off, H, W), a in zip(entries, images):
        arena[off:off + a.size] = a.reshape(-1)
    return arena, entries


def fetch(arena, entries, i, bug=None):
    """image clamp(i) of the set as [H][W][3]; an entry that reaches outside the arena reads as zeros"""
    n = len(entries)
    i = min(max(int(i), 0), n - 1)
    off, H, W = entries[i]
    if H < 1 or W < 1 or off > arena.size or 3 * H * W > arena.size - off:
        return np.zeros((1, 1, 3), dtype=np.uint8)
    pitch = 3 * W
    if bug == "neighbour_base":
        off = entries[(i + 1) % n][0]
    if bug == "wrong_pitch":
        pitch = 3 * entries[(i + 1) % n][2]
    y, x, c = np.mgrid[0:H, 0:W, 0:3]
    return arena[np.clip(off + y * pitch + x * 3 + c, 0, arena.size - 1)]


# ---- resampling without the cap ----------------------------------------------------------------------------------------------------------------
def resample(img, r, S, bug=None):
    """uint8 [H0][W0][3], a row -> the uint8 window [S][S][3] before the flip: horizontal pass, uint8, vertical pass"""
    img = np.asarray(img)
    ty = [M.coeffs(r["h"], r["Rh"], r["oy"] + j, r["filter"]) for j in range(S)]
    tx = [M.coeffs(r["w"], r["Rw"], r["ox"] + j, r["filter"]) for j in range(S)]
    assert max(len(w) for _, w in ty + tx) <= TAPS_MAX
    if bug == "weights_cut" or (bug == "kind_wrong_axis" and not is_wide(r, bug)):      # the narrow kernel on a sample that is not its own
        ty, tx = [(f, w[:TAPS]) for f, w in ty], [(f, w[:TAPS]) for f, w in tx]
    ylo, yhi = min(f for f, _ in ty), max(f + len(w) for f, w in ty)
    xlo, xhi = min(f for f, _ in tx), max(f + len(w) for f, w in tx)
    box = M._pixels(img, r["y0"] + np.arange(ylo, yhi), r["x0"] + np.arange(xlo, xhi))
    ty = [(f - ylo, w) for f, w in ty]
    tx = [(f - xlo, w) for f, w in tx]
    if bug == "no_intermediate":
        mid = M._pass(box, tx, 1, exact_intermediate=False)
        return np.clip(np.floor(M._pass(mid, ty, 0, exact_intermediate=False) + 0.5), 0, 255).astype(np.uint8)
    return M._pass(M._pass(box, tx, 1), ty, 0).astype(np.uint8)


def window(arena, entries, i, r, S, bug=None):
    return resample(fetch(arena, entries, i, bug), r, S, bug)


def sample(arena, entries, i, r, S, mean, std, seed, b, bug=None):
    """(value [3][S][S], bound [3][S][S]) of sample b made from image i: the window here, flip, normalize and erasing as _augment_model's"""
    return M.sample(None, r, S, mean, std, seed, b, window=window(arena, entries, i, r, S, bug))


def batch(arena, entries, idx, rows, S, mean, std, seed, bug=None):
    out = [sample(arena, entries, i, r, S, mean, std, seed, b, bug) for b, (i, r) in enumerate(zip(idx, rows))]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def eval_geometry(H0, W0, S):
    """torchvision Resize(int(256 / 224 * S)) + CenterCrop(S): (Rh, Rw, oy, ox)"""
    R = int(256 / 224 * S)
    Rh, Rw = (R, int(R * W0 / H0)) if H0 <= W0 else (int(R * H0 / W0), R)
    return Rh, Rw, int(round((Rh - S) / 2.)), int(round((Rw - S) / 2.))


# ---- the golden file: _augment_model's case layout, every source an array [1][H][W][3] of its own size ---------------------------------------
def golden_set(g):
    """(images [uint8 [H][W][3]] in the order of g["sources"], cases [(image index, row, S, PIL's window)])"""
    images = [g[str(name)][0] for name in g["sources"]]
    return images, [(int(c[0]), r, S, px) for c, (img, r, S, px) in zip(g["cases"], M.golden_cases(g))]
