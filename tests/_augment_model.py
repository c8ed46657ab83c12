"""numpy restatement of the input-augmentation stage (include/devit_hip.h, "Input augmentation"), written from the header's statement and from
PIL's Resample.c, not from the kernels: tests/test_augment_model.py holds it to PIL (tests/golden/augment_pil.npz, and PIL live where it
imports), tests/test_gpu_augment.py holds the kernels to it.

A table row here is a dict with the fields of devit_augment_sample: y0, x0, h, w, Rh, Rw, oy, ox, filter, flip, erase (a list of up to four
(top, left, h, w)), erase_mode, noise_base.

Bounds.  eps = 2^-24 is the unit roundoff of fp32, ulp = 2^-23 bounds one ulp relative to the value.

normalize_bound: the kernel computes fl(fl(fl(u / 255) - m32) / s32) with m32 = fl(mean), s32 = fl(std); the reference is (u / 255 - mean) / std
in float64 on the mean and std as given.  With a = u / 255, d = a - mean, x = d / std, the roundings are: the first division (<= eps a), the
mean's own (<= eps |mean|), the subtraction (<= eps |d|, to first order), each carried through the division by std; then std's own
(<= eps |x|) and the second division (<= eps |x|):
    |err| <= (eps a + eps |mean| + eps |d|) / std + 2 eps |x|,   times (1 + 2^-20) for the second-order terms (each is eps times a term above).
At mean 0.5, std 0.2 that is at most 2.1e-6; neighbouring uint8 levels are 1 / (255 std) >= 1.4e-2 apart, so holding the bound proves the
integer stage exact.

noise_bound: z = r t, r = sqrt(L), L = -2 ln u (or -2 log1p(-(1 - u))), t = cos / sin(pi a).  The inputs u, 1 - u and a are exact in fp32
(the header says why).  The library functions are held to the OpenCL 3.0 full-profile bounds, the public accuracy contract of the device
math library: log and log1p <= 3 ulp, sqrt <= 3 ulp, sinpi and cospi <= 4 ulp.  L is 3 ulp off (times 2 is exact), which the square root halves
(1.5), plus the square root's own 3, the trigonometric factor's 4 and the product's half:
    |err| <= 9 ulp |z| (1 + 2^-20).
"""
import numpy as np

from _philox import philox4x32_10

EPS = 2.0 ** -24
ULP = 2.0 ** -23
SECOND_ORDER = 1.0 + 2.0 ** -20
TAPS, MAX_ERASE, SITE = 12, 4, 0x100
NONE, BILINEAR, BICUBIC = 0, 1, 2
CONST, RAND, PIXEL = 0, 1, 2
NOISE_ULPS = 9


def row(y0, x0, h, w, S, Rh=None, Rw=None, oy=0, ox=0, filter=BICUBIC, flip=0, erase=(), erase_mode=CONST, noise_base=0):
    return dict(y0=y0, x0=x0, h=h, w=w, Rh=S if Rh is None else Rh, Rw=S if Rw is None else Rw, oy=oy, ox=ox, filter=filter, flip=flip,
                erase=[tuple(e) for e in erase], erase_mode=erase_mode, noise_base=noise_base)


# ---- resampling coefficients: python floats are IEEE doubles and nothing here is contracted -----------------------------------------------
def _filter(x, cubic):
    if x < 0.0:
        x = -x
    if cubic:
        a = -0.5
        if x < 1.0:
            return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
        if x < 2.0:
            return (((x - 5) * x + 8) * x - 4) * a
        return 0.0
    return 1.0 - x if x < 1.0 else 0.0


def coeffs(length, R, xx, filt, in0=0, limit=None):
    """(xmin, [integer weights]) of virtual output index xx.  in0 / limit: the planted bug only (taps over the whole axis, as resize(box=) does)."""
    if filt == NONE:
        return xx, [1 << 22]
    cubic = filt == BICUBIC
    scale = float(length) / float(R)
    fs = 1.0 if scale < 1.0 else scale
    support = (2.0 if cubic else 1.0) * fs
    center = in0 + (xx + 0.5) * scale
    ss = 1.0 / fs
    xmin = max(int(center - support + 0.5), 0)
    xmax = min(int(center + support + 0.5), length if limit is None else limit)
    w = [_filter((k + xmin - center + 0.5) * ss, cubic) for k in range(xmax - xmin)]
    ww = 0.0
    for v in w:
        ww += v
    if ww != 0.0:
        w = [v / ww for v in w]
    return xmin, [int(-0.5 + v * (1 << 22)) if v < 0 else int(0.5 + v * (1 << 22)) for v in w]


def taps_needed(length, R, filt):
    """the most taps any output index of the axis uses (what a loader refuses above TAPS)"""
    return max(len(coeffs(length, R, xx, filt)[1]) for xx in range(R))


def _pixels(img, ys, xs):
    """img[ys][:, xs] with 0 outside the image (ys, xs integer arrays of source coordinates)"""
    H, W = img.shape[:2]
    ok = ((ys >= 0) & (ys < H))[:, None] & ((xs >= 0) & (xs < W))[None, :]
    v = img[np.clip(ys, 0, H - 1)][:, np.clip(xs, 0, W - 1)].astype(np.int64)
    return v * ok[:, :, None]


def _pass(a, table, axis, exact_intermediate=True):
    """one resampling pass along `axis` of a [rows][cols][3] array: table = [(first index into a, weights)] per output index"""
    a = np.moveaxis(a, axis, 0)
    out = []
    for first, w in table:
        acc = np.full(a.shape[1:], 1 << 21, dtype=np.int64) if exact_intermediate else np.zeros(a.shape[1:])
        for k, wk in enumerate(w):
            acc = acc + a[first + k] * wk
        out.append(np.clip(acc >> 22, 0, 255) if exact_intermediate else acc / float(1 << 22))
    return np.moveaxis(np.stack(out), 0, axis)


def resample(img, r, S, bug=None):
    """uint8 [H0][W0][3], a row -> the uint8 window [S][S][3] before the flip.  bug: None or one of the planted ones below."""
    img = np.asarray(img)
    H0, W0 = img.shape[:2]
    if bug == "flip_before_crop" and r["flip"]:
        img = img[:, ::-1]
    escape = bug == "taps_escape" and r["filter"] != NONE
    ty = [coeffs(r["h"], r["Rh"], r["oy"] + j, r["filter"], *((r["y0"], H0) if escape else ())) for j in range(S)]
    tx = [coeffs(r["w"], r["Rw"], r["ox"] + j, r["filter"], *((r["x0"], W0) if escape else ())) for j in range(S)]
    assert max(len(w) for _, w in ty + tx) <= TAPS
    oy0, ox0 = (0, 0) if escape else (r["y0"], r["x0"])
    ylo, yhi = min(f for f, _ in ty), max(f + len(w) for f, w in ty)
    xlo, xhi = min(f for f, _ in tx), max(f + len(w) for f, w in tx)
    box = _pixels(img, oy0 + np.arange(ylo, yhi), ox0 + np.arange(xlo, xhi))
    ty = [(f - ylo, w) for f, w in ty]
    tx = [(f - xlo, w) for f, w in tx]
    if bug == "vertical_first":
        return _pass(_pass(box, ty, 0), tx, 1).astype(np.uint8)
    if bug == "no_intermediate":
        mid = _pass(box, tx, 1, exact_intermediate=False)
        return np.clip(np.floor(_pass(mid, ty, 0, exact_intermediate=False) + 0.5), 0, 255).astype(np.uint8)
    return _pass(_pass(box, tx, 1), ty, 0).astype(np.uint8)


# ---- noise ---------------------------------------------------------------------------------------------------------------------------------
def _words(seed, N, c, g):
    g = np.asarray(g, dtype=np.uint64)
    return philox4x32_10((np.uint64(N & 0xFFFFFFFF), np.uint64((N >> 32) & 0xFFFFFFFF), np.uint64(SITE + c), g), (seed & 0xFFFFFFFF, seed >> 32))


def _u(w):
    return ((w >> np.uint32(8)).astype(np.float64) + 0.5) * 2.0 ** -24


def normals4(seed, N, c, g, fp32=False):
    """[4][len(g)] normals of counter (N, SITE + c, g): float64 from the definition, or (fp32) an emulation that rounds every library function's
    exact result and every product to fp32 -- the arithmetic the kernel is allowed"""
    w = _words(seed, N, c, g)
    z = []
    for p in (0, 2):
        L = -2.0 * np.log(_u(w[p]))
        t = 2.0 * np.pi * _u(w[p + 1])
        if fp32:
            r = np.sqrt(L.astype(np.float32).astype(np.float64)).astype(np.float32)
            z += [r * np.cos(t).astype(np.float32), r * np.sin(t).astype(np.float32)]
        else:
            z += [np.sqrt(L) * np.cos(t), np.sqrt(L) * np.sin(t)]
    return np.stack(z)


def noise_bound(z):
    return NOISE_ULPS * ULP * np.abs(z) * SECOND_ORDER


# ---- normalization -----------------------------------------------------------------------------------------------------------------------
def normalize(u8, mean, std, fp32=False):
    """[S][S][3] uint8 -> [3][S][S]: float64 on mean / std as given, or the kernel's fp32 statement"""
    if fp32:
        m, s = np.asarray(mean, np.float32), np.asarray(std, np.float32)
        return np.moveaxis((u8.astype(np.float32) / np.float32(255) - m) / s, 2, 0)
    return np.moveaxis((u8.astype(np.float64) / 255.0 - np.asarray(mean, np.float64)) / np.asarray(std, np.float64), 2, 0)


def normalize_bound(u8, mean, std):
    a = u8.astype(np.float64) / 255.0
    mean, std = np.asarray(mean, np.float64), np.asarray(std, np.float64)
    d = a - mean
    x = d / std
    return np.moveaxis(((EPS * a + EPS * np.abs(mean) + EPS * np.abs(d)) / std + 2 * EPS * np.abs(x)) * SECOND_ORDER, 2, 0)


# ---- the whole stage -----------------------------------------------------------------------------------------------------------------------
def erase_masks(r, S):
    """bool [n_erase][S][S] of the row's boxes"""
    yy, xx = np.arange(S)[:, None], np.arange(S)[None, :]
    return [(yy >= t) & (yy < t + h) & (xx >= l) & (xx < l + w) for t, l, h, w in r["erase"]]


def sample(img, r, S, mean, std, seed, b, fp32=False, bug=None, window=None):
    """(value [3][S][S], bound [3][S][S]) of one sample; window: a precomputed uint8 result of resample() (PIL's, from the golden)"""
    u8 = resample(img, r, S, bug) if window is None else window
    if r["flip"] and bug != "flip_before_crop":
        u8 = u8[:, ::-1]
    val, bound = normalize(u8, mean, std, fp32).astype(np.float64), normalize_bound(u8, mean, std)
    N = (r["noise_base"] + b) & 0xFFFFFFFFFFFFFFFF
    for e, m in enumerate(erase_masks(r, S)):
        for c in range(3):
            cn = (c + 1) % 3 if bug == "wrong_channel" else c
            if r["erase_mode"] == CONST:
                z = np.zeros((S, S))
            elif r["erase_mode"] == RAND:
                z = np.full((S, S), normals4(seed, N, cn, [0x80000000 + e], fp32)[0, 0], dtype=np.float64)
            else:
                p = np.arange(S * S)
                z4 = normals4(seed, N, cn, p >> 2, fp32).astype(np.float64)
                z = z4[p & 3, p].reshape(S, S)
            if bug == "erase_before_normalize":
                z = (z - mean[c]) / std[c]
            val[c] = np.where(m, z, val[c])
            bound[c] = np.where(m, noise_bound(z), bound[c])
    return val, bound


def batch(src, idx, rows, S, mean, std, seed, fp32=False, bug=None):
    out = [sample(src[i], r, S, mean, std, seed, b, fp32, bug) for b, (i, r) in enumerate(zip(idx, rows))]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


# ---- the golden file -----------------------------------------------------------------------------------------------------------------------
CASE_FIELDS = ("src", "index", "y0", "x0", "h", "w", "Rh", "Rw", "oy", "ox", "filter", "S", "offset")


def golden_cases(g):
    """[(source image uint8 [H0][W0][3], row, S, PIL's window uint8 [S][S][3])] of tests/golden/augment_pil.npz (already loaded)"""
    out = []
    for c in g["cases"]:
        f = dict(zip(CASE_FIELDS, (int(v) for v in c)))
        S = f["S"]
        img = g[str(g["sources"][f["src"]])][f["index"]]
        r = row(f["y0"], f["x0"], f["h"], f["w"], S, f["Rh"], f["Rw"], f["oy"], f["ox"], f["filter"])
        out.append((img, r, S, g["pixels"][f["offset"]:f["offset"] + S * S * 3].reshape(S, S, 3)))
    return out
