"""Device-resident datasets ("Device-resident datasets"): the whole uint8 image set lives in HBM, the host draws one small
parameter row per sample, and one HIP stage (csrc/augment.hip: devit_augment_batch) turns a batch of indices into the normalized fp32
batch [B,3,S,S] that Mixup and the patch-row kernels consume.  It stands where the reference has a DataLoader over
timm.data.transforms_factory.transforms_imagenet_train / the Resize + CenterCrop eval stack (data/get_dataset.py:71-109): crop and resize
(or the padded crop at 32 pixels), horizontal flip, RandAugment's `rand-...-inc1` layers or ColorJitter without hue on the uint8 window
(devit_augment_batch_ops; the header's "Image ops"), ToTensor, Normalize, RandomErasing.

A set whose images differ in size is held packed (DeviceImageSet's `.ragged` form: one byte arena and a directory of offsets and sizes;
devit_augment_ragged, the header's "Packed sets"): every sample is then drawn and resized on its own image's size, crops up to 128 taps.

The draws are timm 0.5.4's own scalar formulas on a private random.Random; the arithmetic is the header's ("Input augmentation").
Nothing here imports torchvision or timm; PIL only to read an image folder."""
import math
import os
import pickle
import random

import numpy as np
import torch

from . import _lib as L
from . import ops
from ._lib import ptr, stream_ptr

IMAGENET_DEFAULT_MEAN = (0.485, 0.456, 0.406)
IMAGENET_DEFAULT_STD = (0.229, 0.224, 0.225)

# host mirror of devit_augment_sample (120 bytes, _lib.AugmentSample)
AUG_SAMPLE_DTYPE = np.dtype([(n, "<i4") for n in ("y0", "x0", "h", "w", "Rh", "Rw", "oy", "ox", "filter", "flip", "n_erase", "erase_mode")] +
                            [("erase", "<i4", (4, 4)), ("noise_base", "<u8")])
# host mirror of devit_augment_ops (328 bytes, _lib.AugmentOps): a sample's image-op layers
AUG_OPS_DTYPE = np.dtype([("n_ops", "<i4"), ("reserved", "<i4"), ("op", "<i4", (4,)), ("filter", "<i4", (4,)), ("factor", "<f4", (4,)),
                          ("arg", "<i4", (4,)), ("fill", "<i4", (4, 4)), ("matrix", "<f8", (4, 6))])
FILTERS = {"bilinear": L.AUG_BILINEAR, "bicubic": L.AUG_BICUBIC}
ERASE_MODES = {"const": L.AUG_ERASE_CONST, "rand": L.AUG_ERASE_RAND, "pixel": L.AUG_ERASE_PIXEL}
# host mirror of devit_image_entry (16 bytes, _lib.ImageEntry): one image of a packed set
IMAGE_ENTRY_DTYPE = np.dtype([("offset", "<u8"), ("H", "<i4"), ("W", "<i4")])
ARENA_ALIGN = 16                      # every image of a packed set starts at a multiple of this
RESIDENT_RESERVE_BYTES = 8 << 30      # of the device's free memory left to the models, activations and workspaces when a folder is made resident
DECODE_WORKERS = 16                   # threads that decode a folder's images, at most
IMG_EXTENSIONS = ('.jpg', '.jpeg', '.png', '.ppm', '.bmp', '.pgm', '.tif', '.tiff', '.webp')      # torchvision's ImageFolder list


def taps_needed(length, R, filt):
    """The most taps one output index of an axis uses when `length` source pixels are resized to R (the header's xmax - xmin)."""
    if filt == L.AUG_NONE:
        return 1
    scale = length / R
    support = (2.0 if filt == L.AUG_BICUBIC else 1.0) * max(scale, 1.0)
    most = 0
    for xx in range(R):
        center = (xx + 0.5) * scale
        most = max(most, min(int(center + support + 0.5), length) - max(int(center - support + 0.5), 0))
    return most


def _check_taps(length, R, filt, what):
    n = taps_needed(length, R, filt)
    if n > L.AUGMENT_TAPS:
        name = {v: k for k, v in FILTERS.items()}[filt]
        raise ValueError(f"{what}: resizing {length} source pixels to {R} with the {name} filter needs {n} taps per output pixel, the resampling "
                         f"kernel holds {L.AUGMENT_TAPS} (a crop side up to 3 x the output side for bicubic, 6 x for bilinear)")


def taps_bound(length, R, filt):
    """The header's closed-form bound on taps_needed ("Packed sets"), on numpy arrays: min(floor(2 * support) + 1, length), 1 for filter 0.
    Never below the exact count and at most 1 above it; it is what the kernels decide a sample's kind with."""
    length, R, filt = np.broadcast_arrays(np.asarray(length, np.int64), np.asarray(R, np.int64), np.asarray(filt, np.int64))
    res = (filt != L.AUG_NONE) & (length > 0) & (R > 0)
    scale = length.astype(np.float64) / np.where(res, R, 1).astype(np.float64)
    support = np.where(filt == L.AUG_BICUBIC, 2.0, 1.0) * np.maximum(scale, 1.0)
    return np.where(res, np.minimum(np.floor(2.0 * support) + 1.0, length.astype(np.float64)), 1.0).astype(np.int64)


def _exact_where_over(bound, length, R, filt):
    """bound with every entry above the wide kernel's limit replaced by the exact count (the bound may be 1 above it: only there does it matter)"""
    bound = np.array(bound, dtype=np.int64)
    length, R, filt = np.broadcast_arrays(length, R, filt)
    for i in np.flatnonzero(bound > L.AUGMENT_TAPS_MAX):
        bound[i] = taps_needed(int(length[i]), int(R[i]), int(filt[i]))
    return bound


def parse_auto_augment(config):
    """timm's RandAugment config string 'rand-m<int>-mstd<float>-inc<0|1>-n<int>' -> dict(m, n, mstd) (defaults m 10, n 2, mstd 0).  Only the
    `inc1` operation set is built; ValueError names what a string asks for beyond that."""
    parts = str(config).split("-")
    if parts[0] != "rand":
        what = {"augmix": "AugMix", "original": "the AutoAugment policy 'original'", "originalr": "the AutoAugment policy 'originalr'",
                "v0": "the AutoAugment policy 'v0'", "v0r": "the AutoAugment policy 'v0r'"}.get(parts[0], f"the policy {parts[0]!r}")
        raise ValueError(f"auto_augment {config!r}: {what} is not built, only RandAugment's rand-m<M>-mstd<F>-inc1-n<N>")
    out, inc = {"m": 10, "n": 2, "mstd": 0.0}, 0
    for part in parts[1:]:
        try:
            if part.startswith("mstd"):
                out["mstd"] = float(part[4:])
            elif part.startswith("inc"):
                inc = int(bool(int(part[3:])))
            elif part.startswith("m"):
                out["m"] = int(part[1:])
            elif part.startswith("n"):
                out["n"] = int(part[1:])
            elif part.startswith("w"):
                raise ValueError(f"auto_augment {config!r}: the weighted op choice ({part}) is not built")
            else:
                raise ValueError(f"auto_augment {config!r}: unknown section {part!r} (m<int>, mstd<float>, inc1, n<int>)")
        except ValueError as e:
            if "auto_augment" in str(e):
                raise
            raise ValueError(f"auto_augment {config!r}: section {part!r} does not parse (m<int>, mstd<float>, inc1, n<int>)")
    if not inc:
        raise ValueError(f"auto_augment {config!r}: the non-increasing op set (inc0, timm's default) is not built: add -inc1")
    if not 1 <= out["n"] <= L.AUGMENT_MAX_OPS:
        raise ValueError(f"auto_augment {config!r}: n = {out['n']}: the op stage holds 1 .. {L.AUGMENT_MAX_OPS} layers per sample")
    if out["m"] < 0 or not out["mstd"] >= 0:
        raise ValueError(f"auto_augment {config!r}: m and mstd must not be negative")
    return out


def rotate_matrix(deg, S):
    """PIL's Image.rotate(deg) about the centre of an S x S image, as the six doubles of Image.transform(AFFINE)"""
    t = -math.radians(deg % 360.0)
    m = [round(math.cos(t), 15), round(math.sin(t), 15), 0.0, round(-math.sin(t), 15), round(math.cos(t), 15), 0.0]
    c = S / 2.0
    m[2] = m[0] * (-c) + m[1] * (-c) + m[2] + c
    m[5] = m[3] * (-c) + m[4] * (-c) + m[5] + c
    return m


# ---- the resident set ------------------------------------------------------------------------------------------------------------------------
def pack_images(arrays):
    """[uint8 [H,W,3]] -> (arena uint8 [bytes], IMAGE_ENTRY_DTYPE [n]): the images HWC one behind the other, each at a multiple of ARENA_ALIGN"""
    entries = np.zeros(len(arrays), dtype=IMAGE_ENTRY_DTYPE)
    at = 0
    for i, a in enumerate(arrays):
        if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.shape[0] < 1 or a.shape[1] < 1:
            raise ValueError(f"DeviceImageSet: image {i} must be uint8 [H,W,3] with H, W >= 1, got {a.dtype} {tuple(a.shape)}")
        entries[i] = (at, a.shape[0], a.shape[1])
        at += (a.size + ARENA_ALIGN - 1) // ARENA_ALIGN * ARENA_ALIGN
    arena = np.zeros(at, dtype=np.uint8)
    for e, a in zip(entries, arrays):
        arena[int(e["offset"]):int(e["offset"]) + a.size] = a.reshape(-1)
    return arena, entries


def check_directory(entries, arena_bytes):
    """ValueError for a directory the kernels would read as zeros or that aliases images: H, W >= 1, offset + 3 H W <= arena_bytes, no overlap"""
    if entries.dtype != IMAGE_ENTRY_DTYPE or entries.ndim != 1 or entries.shape[0] < 1:
        raise ValueError("DeviceImageSet: the directory is a 1-d numpy array of IMAGE_ENTRY_DTYPE with at least one entry")
    H, W, off = entries["H"].astype(np.int64), entries["W"].astype(np.int64), entries["offset"]
    bad = np.flatnonzero((H < 1) | (W < 1))
    if bad.size:
        raise ValueError(f"DeviceImageSet: image {bad[0]} is {H[bad[0]]} x {W[bad[0]]}: H, W >= 1")
    if (H > 1 << 20).any() or (W > 1 << 20).any():
        raise ValueError("DeviceImageSet: an image side above 2^20 pixels")
    end = off + (3 * H * W).astype(np.uint64)
    bad = np.flatnonzero((off > np.uint64(arena_bytes)) | (end > np.uint64(arena_bytes)))
    if bad.size:
        raise ValueError(f"DeviceImageSet: image {bad[0]} ({H[bad[0]]} x {W[bad[0]]} at offset {off[bad[0]]}) reaches past the arena's {arena_bytes} bytes")
    order = np.argsort(off, kind="stable")
    over = np.flatnonzero(end[order][:-1] > off[order][1:])
    if over.size:
        raise ValueError(f"DeviceImageSet: images {order[over[0]]} and {order[over[0] + 1]} overlap in the arena")


class DeviceImageSet:
    """labels int64 [n] on the device, classes: the class names, and the images in one of two forms.
    uniform: images uint8 [n,H0,W0,3] on the device, every image H0 x W0 (`.size`).
    packed (`.ragged`; images of mixed sizes): arena uint8 [bytes] on the device, the images HWC one behind the other at multiples of 16;
    entries: the device directory, one devit_image_entry per image, as uint8 [n * 16]; sizes int32 [n,2] (H, W) on the host."""

    def __init__(self, images, labels, classes, arena=None, entries=None, sizes=None):
        self.images, self.labels, self.classes = images, labels, list(classes)
        self.arena, self.entries, self.sizes = arena, entries, sizes

    def __len__(self):
        return self.labels.shape[0]

    @property
    def ragged(self):
        return self.arena is not None

    @property
    def device(self):
        return self.labels.device

    @property
    def size(self):
        if self.ragged:
            raise ValueError("DeviceImageSet.size: a packed set has one size per image (.sizes)")
        return int(self.images.shape[1]), int(self.images.shape[2])

    @classmethod
    def from_packed(cls, arena, entries, labels, classes=None, device="cuda"):
        """arena uint8 [bytes] and entries IMAGE_ENTRY_DTYPE [n] on the host: the directory is validated here, once, then both go to the device"""
        arena, entries = np.asarray(arena), np.ascontiguousarray(entries)
        if arena.dtype != np.uint8 or arena.ndim != 1:
            raise ValueError(f"DeviceImageSet: the arena must be uint8 [bytes], got {arena.dtype} {tuple(arena.shape)}")
        check_directory(entries, arena.shape[0])
        labels = labels if isinstance(labels, torch.Tensor) else torch.from_numpy(np.asarray(labels, dtype=np.int64))
        if labels.dim() != 1 or labels.shape[0] != entries.shape[0]:
            raise ValueError(f"DeviceImageSet: {entries.shape[0]} images, labels of shape {tuple(labels.shape)}")
        if classes is None:
            classes = [str(i) for i in range(int(labels.max()) + 1)]
        sizes = np.stack([entries["H"], entries["W"]], axis=1).astype(np.int32)
        return cls(None, labels.long().to(device), classes, arena=torch.from_numpy(arena).to(device),
                   entries=torch.from_numpy(entries.view(np.uint8).reshape(-1).copy()).to(device), sizes=sizes)

    @classmethod
    def from_arrays(cls, images, labels, classes=None, device="cuda", ragged=False):
        """ragged: False -- a uniform set, refusing images of differing shapes; True -- a packed set; "auto" -- uniform when every shape agrees"""
        if ragged and isinstance(images, (list, tuple)):
            arrays = [np.asarray(a) for a in images]
            if ragged != "auto" or len({a.shape for a in arrays}) > 1:
                return cls.from_packed(*pack_images(arrays), labels, classes, device)
        elif ragged and ragged != "auto":
            return cls.from_packed(*pack_images(list(np.asarray(images.cpu() if isinstance(images, torch.Tensor) else images))), labels, classes, device)
        if isinstance(images, (list, tuple)):
            shapes = sorted({tuple(np.shape(a)) for a in images})
            if len(shapes) > 1:
                raise ValueError(f"DeviceImageSet: images of shapes {shapes[:4]}: resident sets are uniform (one H x W for every image)")
            images = np.stack([np.asarray(a) for a in images])
        images = images if isinstance(images, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(images))
        labels = labels if isinstance(labels, torch.Tensor) else torch.from_numpy(np.asarray(labels, dtype=np.int64))
        if images.dtype != torch.uint8 or images.dim() != 4 or images.shape[3] != 3:
            raise ValueError(f"DeviceImageSet: images must be uint8 [n,H,W,3], got {images.dtype} {tuple(images.shape)}")
        if labels.dim() != 1 or labels.shape[0] != images.shape[0] or images.shape[0] < 1:
            raise ValueError(f"DeviceImageSet: {images.shape[0]} images, labels of shape {tuple(labels.shape)}")
        if classes is None:
            classes = [str(i) for i in range(int(labels.max()) + 1)]
        return cls(images.contiguous().to(device), labels.long().to(device), classes)

    @classmethod
    def from_cifar100(cls, root, train, device="cuda"):
        """The `cifar-100-python` pickles under root (what torchvision's CIFAR100 unpacks), read with pickle and numpy."""
        path = os.path.join(root, "cifar-100-python", "train" if train else "test")
        if not os.path.exists(path):
            raise SystemExit(f"--device-data: {path} not found (the cifar-100-python pickles under --data-path)")
        with open(path, "rb") as f:
            d = pickle.load(f, encoding="latin1")
        images = np.ascontiguousarray(np.asarray(d["data"], dtype=np.uint8).reshape(-1, 3, 32, 32).transpose(0, 2, 3, 1))
        meta = os.path.join(root, "cifar-100-python", "meta")
        classes = None
        if os.path.exists(meta):
            with open(meta, "rb") as f:
                classes = list(pickle.load(f, encoding="latin1")["fine_label_names"])
        return cls.from_arrays(images, np.asarray(d["fine_labels"], dtype=np.int64), classes or [str(i) for i in range(100)], device)

    @classmethod
    def from_folder(cls, root, device="cuda", ragged=False, budget_bytes=None):
        """An ImageFolder tree root/<class>/<file>: classes are the sorted directory names, files sorted within a class, read with PIL
        and convert('RGB').  ragged (True or "auto", as from_arrays): a first pass reads the headers only, adds up the bytes and refuses
        with SystemExit, before any image is decoded, a set above budget_bytes (None: the device's free memory less RESIDENT_RESERVE_BYTES);
        then the images are decoded straight into the arena by at most DECODE_WORKERS threads."""
        try:
            from PIL import Image
        except ImportError as e:
            raise SystemExit("DeviceImageSet.from_folder reads images with PIL, which is not installed: " + repr(e))
        if not os.path.isdir(root):
            raise SystemExit(f"--device-data: {root} is not a directory (an ImageFolder tree, as splite_dataset.py writes)")
        classes = sorted(d for d in os.listdir(root) if os.path.isdir(os.path.join(root, d)))
        if ragged:
            return cls._from_folder_packed(Image, root, classes, device, ragged, budget_bytes)
        images, labels, size = [], [], None
        for ci, c in enumerate(classes):
            for dirpath, _, files in sorted(os.walk(os.path.join(root, c), followlinks=True)):
                for fn in sorted(files):
                    if not fn.lower().endswith(IMG_EXTENSIONS):
                        continue
                    with Image.open(os.path.join(dirpath, fn)) as im:
                        a = np.asarray(im.convert('RGB'), dtype=np.uint8)
                    if size is None:
                        size = a.shape[:2]
                    if a.shape[:2] != size:
                        raise ValueError(f"{os.path.join(dirpath, fn)} is {a.shape[0]} x {a.shape[1]}, the images before it {size[0]} x {size[1]}: "
                                         "resident sets are uniform (one H x W for every image)")
                    images.append(a)
                    labels.append(ci)
        if not images:
            raise SystemExit(f"--device-data: no images under {root}")
        return cls.from_arrays(np.stack(images), np.asarray(labels, dtype=np.int64), classes, device)

    @classmethod
    def _from_folder_packed(cls, Image, root, classes, device, ragged, budget_bytes):
        from concurrent.futures import ThreadPoolExecutor
        paths, labels = [], []
        for ci, c in enumerate(classes):
            for dirpath, _, files in sorted(os.walk(os.path.join(root, c), followlinks=True)):
                for fn in sorted(files):
                    if fn.lower().endswith(IMG_EXTENSIONS):
                        paths.append(os.path.join(dirpath, fn))
                        labels.append(ci)
        if not paths:
            raise SystemExit(f"--device-data: no images under {root}")
        entries = np.zeros(len(paths), dtype=IMAGE_ENTRY_DTYPE)
        at = 0
        for i, p in enumerate(paths):               # the headers only: nothing is decoded
            with Image.open(p) as im:
                W, H = im.size
            entries[i] = (at, H, W)
            at += (3 * H * W + ARENA_ALIGN - 1) // ARENA_ALIGN * ARENA_ALIGN
        free = None
        if budget_bytes is None and torch.device(device).type == "cuda":
            free = torch.cuda.mem_get_info(device)[0]
            budget_bytes = free - RESIDENT_RESERVE_BYTES
        if budget_bytes is not None and at > budget_bytes:
            big = int(np.argmax(entries["H"].astype(np.int64) * entries["W"]))
            raise SystemExit(f"--device-data: the {len(paths)} images under {root} take {at} bytes as uint8, the budget for a resident set is {budget_bytes} bytes "
                             + (f"(the device's {free} free bytes less a reserve of {RESIDENT_RESERVE_BYTES} for the models and activations)" if free is not None
                                else "(budget_bytes)")
                             + f"; the largest image is {paths[big]}, {entries['H'][big]} x {entries['W'][big]}")
        uniform = ragged == "auto" and len(set(zip(entries["H"].tolist(), entries["W"].tolist()))) == 1
        arena = np.zeros(at, dtype=np.uint8)

        def decode(i):
            with Image.open(paths[i]) as im:
                a = np.asarray(im.convert('RGB'), dtype=np.uint8)
            H, W = int(entries["H"][i]), int(entries["W"][i])
            if a.shape != (H, W, 3):
                raise ValueError(f"{paths[i]} decodes to {a.shape[0]} x {a.shape[1]}, its header says {H} x {W}")
            arena[int(entries["offset"][i]):int(entries["offset"][i]) + a.size] = a.reshape(-1)
        with ThreadPoolExecutor(max_workers=DECODE_WORKERS) as pool:
            list(pool.map(decode, range(len(paths))))
        labels = np.asarray(labels, dtype=np.int64)
        if uniform:
            H, W = int(entries["H"][0]), int(entries["W"][0])
            step = (3 * H * W + ARENA_ALIGN - 1) // ARENA_ALIGN * ARENA_ALIGN
            return cls.from_arrays(np.ascontiguousarray(arena.reshape(len(paths), step)[:, :3 * H * W]).reshape(len(paths), H, W, 3), labels, classes, device)
        return cls.from_packed(arena, entries, labels, classes, device)

    def save(self, path):
        """The set as plain arrays under directory `path`: arena.npy + entries.npy (packed) or images.npy (uniform), labels.npy, classes.npy"""
        os.makedirs(path, exist_ok=True)
        if self.ragged:
            np.save(os.path.join(path, "arena.npy"), self.arena.cpu().numpy())
            np.save(os.path.join(path, "entries.npy"), self.entries.cpu().numpy().view(IMAGE_ENTRY_DTYPE))
        else:
            np.save(os.path.join(path, "images.npy"), self.images.cpu().numpy())
        np.save(os.path.join(path, "labels.npy"), self.labels.cpu().numpy())
        np.save(os.path.join(path, "classes.npy"), np.array([str(c) for c in self.classes], dtype=np.str_))

    @classmethod
    def load(cls, path, device="cuda"):
        """What save() wrote; the image bytes are mapped (copy-on-write), so they are read once, by the copy to the device"""
        labels = np.load(os.path.join(path, "labels.npy"))
        classes = [str(c) for c in np.load(os.path.join(path, "classes.npy"))]
        if os.path.exists(os.path.join(path, "arena.npy")):
            return cls.from_packed(np.load(os.path.join(path, "arena.npy"), mmap_mode="c"), np.load(os.path.join(path, "entries.npy")), labels, classes, device)
        return cls.from_arrays(torch.from_numpy(np.load(os.path.join(path, "images.npy"), mmap_mode="c")), labels, classes, device)

    @staticmethod
    def saved(path):
        return os.path.exists(os.path.join(path, "labels.npy"))


# ---- the per-sample draws --------------------------------------------------------------------------------------------------------------------
def _per_sample(B, H0, W0):
    """H0, W0 as ints (every sample's) or as int arrays of length B -> two lists of B python ints"""
    out = []
    for v in (H0, W0):
        if np.ndim(v) == 0:
            out.append([int(v)] * B)
        else:
            if len(v) != B:
                raise ValueError(f"draw: {len(v)} image sizes for {B} samples")
            out.append([int(x) for x in v])
    return out


def _refuse_over_wide(who, H, W, need):
    """ValueError naming the images (index, size) whose `need` taps exceed the wide kernel's limit"""
    bad = np.flatnonzero(need > L.AUGMENT_TAPS_MAX)
    if bad.size:
        some = ", ".join(f"image {i} ({H[i]} x {W[i]}: {need[i]} taps)" for i in bad[:5])
        raise ValueError(f"{who}: {bad.size} image(s) of the set need more than {L.AUGMENT_TAPS_MAX} taps per output pixel (DEVIT_AUGMENT_TAPS_MAX), "
                         f"the first: {some}")


class TrainAugment:
    """One devit_augment_sample per sample, drawn as timm 0.5.4 draws (transforms_imagenet_train: RandomResizedCropAndInterpolation.get_params,
    the interpolation when 'random', RandomHorizontalFlip, RandomErasing._erase), in that order, on a private random.Random seeded by
    (seed, rank) and carried across epochs.  S == 32: the crop is RandomCrop(S, padding=4) at unit scale (data/get_dataset.py:92-96)."""

    def __init__(self, S, scale=(0.08, 1.0), ratio=(3. / 4., 4. / 3.), interpolation='bicubic', hflip=0.5, re_prob=0., re_mode='const',
                 re_count=1, seed=0, rank=0, mean=IMAGENET_DEFAULT_MEAN, std=IMAGENET_DEFAULT_STD, auto_augment=None, color_jitter=None):
        self.S = ops.check_img_size(S, exc=ValueError)
        self.rand = parse_auto_augment(auto_augment) if auto_augment and auto_augment != 'none' else None
        self.color_jitter = float(color_jitter) if color_jitter and self.rand is None else 0.      # timm: if auto_augment ... elif color_jitter
        if self.color_jitter < 0:
            raise ValueError(f"TrainAugment: color_jitter {color_jitter} must not be negative")
        if interpolation != 'random' and interpolation not in FILTERS:
            raise ValueError(f"TrainAugment: interpolation {interpolation!r}: bicubic, bilinear or random")
        re_mode = re_mode or 'const'
        if re_mode not in ERASE_MODES:
            raise ValueError(f"TrainAugment: re_mode {re_mode!r}: const, rand or pixel")
        if not 1 <= re_count <= L.AUGMENT_MAX_ERASE:
            raise ValueError(f"TrainAugment: re_count {re_count}: the erase stage holds 1 .. {L.AUGMENT_MAX_ERASE} boxes per sample")
        self.scale, self.ratio, self.interpolation, self.hflip = tuple(scale), tuple(ratio), interpolation, hflip
        self.re_prob, self.re_mode, self.re_count = re_prob, re_mode, re_count
        self.seed, self.rank, self.mean, self.std = int(seed), int(rank), tuple(mean), tuple(std)
        self.fill = tuple(min(255, round(255 * m)) for m in self.mean)
        self.rng = random.Random(self.seed * 65536 + self.rank)
        self.drawn = 0            # samples drawn so far: the noise counter base of the next batch

    @property
    def has_ops(self):
        return self.rand is not None or self.color_jitter > 0

    def check_set(self, H0, W0):
        """Refuse a set this transform cannot serve (the tap limit of the resampling kernel), before anything is drawn.  H0, W0: ints (a
        uniform set) or the int arrays of a packed set's sizes, which the wide kernel serves up to DEVIT_AUGMENT_TAPS_MAX taps."""
        if np.ndim(H0):
            H, W = np.asarray(H0, np.int64), np.asarray(W0, np.int64)
            if self.S == 32:
                bad = np.flatnonzero((H + 8 < self.S) | (W + 8 < self.S))
                if bad.size:
                    raise ValueError(f"TrainAugment: a padded {self.S} x {self.S} crop does not fit image {bad[0]} ({H[bad[0]]} x {W[bad[0]]})")
                return
            need = np.zeros(H.shape[0], np.int64)
            for f in (FILTERS.values() if self.interpolation == 'random' else (FILTERS[self.interpolation],)):
                for side in (H, W):                                  # the largest crop is the whole side
                    need = np.maximum(need, _exact_where_over(taps_bound(side, self.S, f), side, self.S, f))
            _refuse_over_wide(f"TrainAugment at {self.S} pixels", H, W, need)
            return
        if self.S == 32:
            if H0 + 8 < self.S or W0 + 8 < self.S:
                raise ValueError(f"TrainAugment: a padded {self.S} x {self.S} crop does not fit {H0} x {W0} images")
            return
        for f in (FILTERS.values() if self.interpolation == 'random' else (FILTERS[self.interpolation],)):
            _check_taps(H0, self.S, f, f"TrainAugment on {H0} x {W0} images")      # the largest crop is the whole side
            _check_taps(W0, self.S, f, f"TrainAugment on {H0} x {W0} images")

    def _crop(self, H0, W0):
        rng = self.rng
        area = W0 * H0
        for _ in range(10):
            target_area = rng.uniform(*self.scale) * area
            aspect_ratio = math.exp(rng.uniform(math.log(self.ratio[0]), math.log(self.ratio[1])))
            w = int(round(math.sqrt(target_area * aspect_ratio)))
            h = int(round(math.sqrt(target_area / aspect_ratio)))
            if w <= W0 and h <= H0:
                i = rng.randint(0, H0 - h)
                j = rng.randint(0, W0 - w)
                return i, j, h, w
        in_ratio = W0 / H0                    # fallback: the central crop with the ratio clamped
        if in_ratio < min(self.ratio):
            w = W0
            h = int(round(w / min(self.ratio)))
        elif in_ratio > max(self.ratio):
            h = H0
            w = int(round(h * max(self.ratio)))
        else:
            w, h = W0, H0
        return (H0 - h) // 2, (W0 - w) // 2, h, w

    def _erase(self):
        rng, S, boxes = self.rng, self.S, []
        if rng.random() > self.re_prob:
            return boxes
        count = 1 if self.re_count == 1 else rng.randint(1, self.re_count)
        for _ in range(count):
            for _ in range(10):
                target_area = rng.uniform(0.02, 1 / 3) * (S * S) / count
                aspect_ratio = math.exp(rng.uniform(math.log(0.3), math.log(1 / 0.3)))
                h = int(round(math.sqrt(target_area * aspect_ratio)))
                w = int(round(math.sqrt(target_area / aspect_ratio)))
                if w < S and h < S:
                    boxes.append((rng.randint(0, S - h), rng.randint(0, S - w), h, w))
                    break
        return boxes

    def _layers(self):
        """the image-op layers of one sample [(op, filter, factor, arg, matrix)]: RandAugment's n draws (op, applied?, magnitude, sign, filter)
        or ColorJitter's order and factors"""
        rng, S, out = self.rng, self.S, []
        if self.rand is None:
            order = [0, 1, 2]
            rng.shuffle(order)
            cj = self.color_jitter
            f = [rng.uniform(max(0., 1. - cj), 1. + cj) for _ in range(3)]            # brightness, contrast, saturation: timm's argument order
            return [((L.OP_BRIGHTNESS, L.OP_CONTRAST, L.OP_COLOR)[k], L.AUG_BILINEAR, f[k], 0, None) for k in order]
        m, mstd = self.rand["m"], self.rand["mstd"]
        for _ in range(self.rand["n"]):
            op = rng.randrange(L.OP_COUNT)
            if rng.random() > 0.5:
                continue
            mag = float(m)
            if mstd > 0:
                mag = rng.uniform(0, mag) if mstd == float('inf') else rng.gauss(mag, mstd)
            lvl = min(10., max(0., mag)) / 10.
            factor, arg, matrix, filt = 1., 0, None, L.AUG_BILINEAR
            if op in (L.OP_ROTATE, L.OP_SHEAR_X, L.OP_SHEAR_Y, L.OP_TRANSLATE_X, L.OP_TRANSLATE_Y, L.OP_COLOR, L.OP_CONTRAST, L.OP_BRIGHTNESS,
                      L.OP_SHARPNESS):
                v = lvl * {L.OP_ROTATE: 30., L.OP_SHEAR_X: 0.3, L.OP_SHEAR_Y: 0.3, L.OP_TRANSLATE_X: 0.45, L.OP_TRANSLATE_Y: 0.45}.get(op, 0.9)
                if rng.random() > 0.5:
                    v = -v
                if op == L.OP_ROTATE:
                    matrix = rotate_matrix(v, S)
                elif op == L.OP_SHEAR_X:
                    matrix = (1., v, 0., 0., 1., 0.)
                elif op == L.OP_SHEAR_Y:
                    matrix = (1., 0., 0., v, 1., 0.)
                elif op == L.OP_TRANSLATE_X:
                    matrix = (1., 0., v * S, 0., 1., 0.)
                elif op == L.OP_TRANSLATE_Y:
                    matrix = (1., 0., 0., 0., 1., v * S)
                else:
                    factor = 1. + v
                if matrix is not None:
                    filt = rng.choice((L.AUG_BILINEAR, L.AUG_BICUBIC)) if self.interpolation == 'random' else FILTERS[self.interpolation]
            elif op == L.OP_POSTERIZE:
                arg = 4 - int(lvl * 4)
            elif op == L.OP_SOLARIZE:
                arg = 256 - int(lvl * 256)
            elif op == L.OP_SOLARIZE_ADD:
                arg = int(lvl * 110)
            out.append((op, filt, factor, arg, matrix))
        return out

    def draw(self, B, H0, W0):
        """-> AUG_SAMPLE_DTYPE [B]: crop, interpolation if random, flip, erasing per sample (a transform without image-op layers)"""
        if self.has_ops:
            raise ValueError("TrainAugment.draw: this transform draws image-op layers too: draw_with_ops returns both tables")
        return self.draw_with_ops(B, H0, W0)[0]

    def draw_with_ops(self, B, H0, W0):
        """-> (AUG_SAMPLE_DTYPE [B], AUG_OPS_DTYPE [B] or None): crop, interpolation if random, flip, the image-op layers, erasing per sample.
        H0, W0: ints, or int arrays of length B (a packed set): sample b is then drawn on its own size, by the same formulas in the same order."""
        S, rng = self.S, self.rng
        Hs, Ws = _per_sample(B, H0, W0)
        layers = np.zeros(B, dtype=AUG_OPS_DTYPE) if self.has_ops else None
        if layers is not None:
            layers["matrix"][:, :, 0] = layers["matrix"][:, :, 4] = 1.
            layers["fill"][:, :, :3] = self.fill
        cols, erase = [], np.zeros((B, 4, 4), dtype=np.int32)      # (columns are filled at once: a field store per sample costs more than its draw)
        for b in range(B):
            H0, W0 = Hs[b], Ws[b]
            if S == 32:
                y0, x0, h, w, filt = rng.randint(0, H0 + 8 - S) - 4, rng.randint(0, W0 + 8 - S) - 4, S, S, L.AUG_NONE
            else:
                y0, x0, h, w = self._crop(H0, W0)
                if h < 1 or w < 1:
                    raise ValueError(f"TrainAugment: drew an empty {h} x {w} crop on {H0} x {W0} images (scale {self.scale})")
                filt = rng.choice((L.AUG_BILINEAR, L.AUG_BICUBIC)) if self.interpolation == 'random' else FILTERS[self.interpolation]
            flip = int(rng.random() < self.hflip) if self.hflip > 0. else 0
            if layers is not None:
                row = layers[b]
                for k, (op, lf, factor, arg, matrix) in enumerate(self._layers()):
                    row["op"][k], row["filter"][k], row["factor"][k], row["arg"][k] = op, lf, factor, arg
                    if matrix is not None:
                        row["matrix"][k] = matrix
                    row["n_ops"] = k + 1
            boxes = self._erase() if self.re_prob > 0. else ()
            if boxes:
                erase[b, :len(boxes)] = boxes
            cols.append((y0, x0, h, w, filt, flip, len(boxes)))
        tab = np.zeros(B, dtype=AUG_SAMPLE_DTYPE)
        cols = np.asarray(cols, dtype=np.int32)
        for k, name in enumerate(("y0", "x0", "h", "w", "filter", "flip", "n_erase")):
            tab[name] = cols[:, k]
        tab["Rh"], tab["Rw"], tab["erase_mode"], tab["erase"] = S, S, ERASE_MODES[self.re_mode], erase
        tab["noise_base"] = (self.rank << 48) + self.drawn
        self.drawn += B
        return tab, layers

    def state_dict(self):
        return {"rng": self.rng.getstate(), "drawn": self.drawn}

    def load_state_dict(self, state):
        v, words, gauss = state["rng"]
        self.rng.setstate((v, tuple(words), gauss))
        self.drawn = int(state["drawn"])


class EvalTransform:
    """The reference's eval stack (data/get_dataset.py:99-109).  S > 32: torchvision Resize(int(256 / 224 * S)) -- the shorter side to R, the other to
    int(R * long / short), bicubic -- and CenterCrop(S) with offsets int(round((side - S) / 2.)).  S == 32: the image as it is."""

    def __init__(self, S, mean=IMAGENET_DEFAULT_MEAN, std=IMAGENET_DEFAULT_STD):
        self.S, self.seed, self.mean, self.std = ops.check_img_size(S, exc=ValueError), 0, tuple(mean), tuple(std)

    def geometry(self, H0, W0):
        """(Rh, Rw, oy, ox, filter)"""
        S = self.S
        if S == 32:
            return S, S, 0, 0, L.AUG_NONE
        R = int((256 / 224) * S)
        Rh, Rw = (R, int(R * W0 / H0)) if H0 <= W0 else (int(R * H0 / W0), R)
        return Rh, Rw, int(round((Rh - S) / 2.)), int(round((Rw - S) / 2.)), L.AUG_BICUBIC

    def check_set(self, H0, W0):
        if np.ndim(H0):
            H, W = np.asarray(H0, np.int64), np.asarray(W0, np.int64)
            geo = np.asarray([self.geometry(int(h), int(w)) for h, w in zip(H, W)], dtype=np.int64)
            if self.S == 32:
                bad = np.flatnonzero((H != self.S) | (W != self.S))
                if bad.size:
                    raise ValueError(f"EvalTransform: at {self.S} pixels the images are used as they are, and image {bad[0]} is {H[bad[0]]} x {W[bad[0]]}")
                return
            need = np.maximum(_exact_where_over(taps_bound(H, geo[:, 0], geo[:, 4]), H, geo[:, 0], geo[:, 4]),
                              _exact_where_over(taps_bound(W, geo[:, 1], geo[:, 4]), W, geo[:, 1], geo[:, 4]))
            _refuse_over_wide(f"EvalTransform at {self.S} pixels", H, W, need)
            return
        Rh, Rw, _, _, filt = self.geometry(H0, W0)
        if filt == L.AUG_NONE:
            if (H0, W0) != (self.S, self.S):
                raise ValueError(f"EvalTransform: at {self.S} pixels the images are used as they are, and the set's are {H0} x {W0}")
            return
        _check_taps(H0, Rh, filt, f"EvalTransform on {H0} x {W0} images")
        _check_taps(W0, Rw, filt, f"EvalTransform on {H0} x {W0} images")

    def draw(self, B, H0, W0):
        """H0, W0: ints, or int arrays of length B (a packed set): the geometry is then each image's own"""
        tab = np.zeros(B, dtype=AUG_SAMPLE_DTYPE)
        if np.ndim(H0) or np.ndim(W0):
            Hs, Ws = _per_sample(B, H0, W0)
            known = {}
            geo = np.asarray([known.setdefault(hw, self.geometry(*hw)) for hw in zip(Hs, Ws)], dtype=np.int32)
            tab["h"], tab["w"] = Hs, Ws
            for k, name in enumerate(("Rh", "Rw", "oy", "ox", "filter")):
                tab[name] = geo[:, k]
            return tab
        tab["h"], tab["w"] = H0, W0
        tab["Rh"], tab["Rw"], tab["oy"], tab["ox"], tab["filter"] = self.geometry(H0, W0)
        return tab

    def state_dict(self):
        return {}

    def load_state_dict(self, state):
        pass


# ---- the device stage ------------------------------------------------------------------------------------------------------------------------
UPLOAD_RING_SLOTS = 256
_upload_ring = {}     # device -> [pinned uint8 [UPLOAD_RING_SLOTS, bytes per slot], uploads so far] (as ops.mix_table's ring, and for its reason)


def upload(host_bytes, device):
    """numpy uint8 [nbytes] -> a fresh device uint8 tensor through a pinned ring slot of its own, by a copy that never waits for the stream."""
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    nbytes = host_bytes.shape[0]
    ring = _upload_ring.get(device)
    if ring is None or ring[0].shape[1] < nbytes:
        ring = _upload_ring[device] = [torch.zeros((UPLOAD_RING_SLOTS, max(nbytes, 65536)), dtype=torch.uint8).pin_memory(), 0]
    slot = ring[0][ring[1] % UPLOAD_RING_SLOTS, :nbytes]
    ring[1] += 1
    slot.copy_(torch.from_numpy(host_bytes))
    dev = torch.empty(nbytes, dtype=torch.uint8, device=device)
    dev.copy_(slot, non_blocking=True)
    return dev


def check_table(tab, H0, W0, S):
    """ValueError for a table the header's definition does not cover (the kernels are memory-safe for any bytes; this is where values are checked).
    H0, W0 as int arrays, one size per row (a packed set): every row is held to its own image, the tap limit is the wide kernel's, and the
    batch's max_taps for devit_augment_ragged is returned (the header's closed-form bound, in numpy: no loop per distinct length)."""
    ragged = bool(np.ndim(H0) or np.ndim(W0))
    if ragged:
        H0, W0 = np.asarray(H0, np.int64), np.asarray(W0, np.int64)
        if H0.shape != tab.shape or W0.shape != tab.shape:
            raise ValueError(f"augment_batch: {H0.shape[0] if H0.ndim else 1} image sizes for a table of {tab.shape[0]} rows")
    if tab.dtype != AUG_SAMPLE_DTYPE or tab.ndim != 1 or tab.shape[0] < 1:
        raise ValueError("augment_batch: the table is a 1-d numpy array of AUG_SAMPLE_DTYPE")
    filt = tab["filter"]
    if not np.isin(filt, (0, 1, 2)).all() or not np.isin(tab["erase_mode"], (0, 1, 2)).all():
        raise ValueError("augment_batch: filter and erase_mode are 0, 1 or 2")
    if ((tab["n_erase"] < 0) | (tab["n_erase"] > L.AUGMENT_MAX_ERASE)).any():
        raise ValueError(f"augment_batch: n_erase must lie in 0 .. {L.AUGMENT_MAX_ERASE}")
    if ((tab["h"] < 1) | (tab["w"] < 1) | (tab["Rh"] < 1) | (tab["Rw"] < 1)).any():
        raise ValueError("augment_batch: empty box or virtual size")
    if ((tab["oy"] < 0) | (tab["ox"] < 0) | (tab["oy"] + S > tab["Rh"]) | (tab["ox"] + S > tab["Rw"])).any():
        raise ValueError(f"augment_batch: the {S} x {S} window must lie inside the virtual output")
    res = filt != 0
    if (res & ((tab["y0"] < 0) | (tab["x0"] < 0) | (tab["y0"] + tab["h"] > H0) | (tab["x0"] + tab["w"] > W0))).any():
        raise ValueError("augment_batch: a resized box must lie inside its image" if ragged else f"augment_batch: a resized box must lie inside the {H0} x {W0} image")
    if (~res & ((tab["h"] != tab["Rh"]) | (tab["w"] != tab["Rw"]))).any():
        raise ValueError("augment_batch: filter 0 is unit scale: the box has the virtual output's size")
    if ragged:
        need = np.maximum(_exact_where_over(taps_bound(tab["h"], tab["Rh"], filt), tab["h"], tab["Rh"], filt),
                          _exact_where_over(taps_bound(tab["w"], tab["Rw"], filt), tab["w"], tab["Rw"], filt))
        if (need > L.AUGMENT_TAPS_MAX).any():
            b = int(np.argmax(need))
            raise ValueError(f"augment_batch: row {b} resizes a {tab['h'][b]} x {tab['w'][b]} box to {tab['Rh'][b]} x {tab['Rw'][b]}, which needs {need[b]} taps "
                             f"per output pixel; the wide resampling kernel holds {L.AUGMENT_TAPS_MAX}")
        return int(need.max())
    for key in {(int(a), int(b), int(c)) for a, b, c in zip(tab["h"][res], tab["Rh"][res], filt[res])} | \
            {(int(a), int(b), int(c)) for a, b, c in zip(tab["w"][res], tab["Rw"][res], filt[res])}:
        _check_taps(*key, "augment_batch")


def check_ops_table(layers, B):
    """ValueError for an image-op table the header's definition does not cover (the kernel is memory-safe for any bytes, as above)."""
    if layers.dtype != AUG_OPS_DTYPE or layers.ndim != 1 or layers.shape[0] != B:
        raise ValueError(f"image ops: the table is a 1-d numpy array of {B} AUG_OPS_DTYPE rows")
    n = layers["n_ops"]
    if ((n < 0) | (n > L.AUGMENT_MAX_OPS)).any():
        raise ValueError(f"image ops: n_ops must lie in 0 .. {L.AUGMENT_MAX_OPS}")
    live = np.arange(L.AUGMENT_MAX_OPS)[None, :] < n[:, None]
    if (live & ((layers["op"] < 0) | (layers["op"] >= L.OP_COUNT))).any():
        raise ValueError(f"image ops: op ids are 0 .. {L.OP_COUNT - 1}")
    affine = live & np.isin(layers["op"], (L.OP_ROTATE, L.OP_SHEAR_X, L.OP_SHEAR_Y, L.OP_TRANSLATE_X, L.OP_TRANSLATE_Y))
    if (affine & ~np.isin(layers["filter"], (L.AUG_BILINEAR, L.AUG_BICUBIC))).any():
        raise ValueError("image ops: the filter of an affine op is 1 (bilinear) or 2 (bicubic)")
    if (affine & ~np.isfinite(layers["matrix"]).all(axis=2)).any():
        raise ValueError("image ops: the matrix of an affine op must be finite")
    if (live & ~np.isfinite(layers["factor"])).any():
        raise ValueError("image ops: the blend factor must be finite")
    if (live & ((layers["fill"] < 0) | (layers["fill"] > 255)).any(axis=2)).any():
        raise ValueError("image ops: fill levels are 0 .. 255")


def image_ops(images, layers):
    """uint8 [B,S,S,3] on the device, AUG_OPS_DTYPE [B] on the host -> uint8 [B,S,S,3]: the layers alone (devit_image_ops)"""
    L.require_device(images)
    if images.dtype != torch.uint8 or images.dim() != 4 or images.shape[3] != 3 or images.shape[1] != images.shape[2] or not images.is_contiguous():
        raise ValueError(f"image_ops: images must be a contiguous uint8 [B,S,S,3] tensor, got {images.dtype} {tuple(images.shape)}")
    B, S = int(images.shape[0]), ops.check_img_size(int(images.shape[1]), exc=ValueError)
    check_ops_table(layers, B)
    ops_dev = upload(np.ascontiguousarray(layers).view(np.uint8).reshape(-1), images.device)
    out = torch.empty_like(images)
    ops.call("devit_image_ops", ptr(images), ptr(ops_dev), B, S, ptr(out), stream_ptr())
    return out


def augment_batch(src, idx, table, S, mean=IMAGENET_DEFAULT_MEAN, std=IMAGENET_DEFAULT_STD, seed=0, out=None, table_dev=None, layers=None,
                  layers_dev=None):
    """src uint8 [n,H0,W0,3] and idx int32 [B] on the device, table: AUG_SAMPLE_DTYPE [B] on the host (validated here, then uploaded)
    -> fp32 [B,3,S,S] (devit_augment_batch).  table_dev: the table's bytes already on the device (the caller validated and uploaded them).
    layers: AUG_OPS_DTYPE [B], the image-op layers between flip and ToTensor (devit_augment_batch_ops; layers_dev as table_dev)."""
    L.require_device(src)
    if src.dtype != torch.uint8 or src.dim() != 4 or src.shape[3] != 3 or not src.is_contiguous():
        raise ValueError(f"augment_batch: src must be a contiguous uint8 [n,H0,W0,3] tensor, got {src.dtype} {tuple(src.shape)}")
    if idx.dtype != torch.int32 or idx.dim() != 1 or idx.device != src.device or not idx.is_contiguous():
        raise ValueError("augment_batch: idx must be a contiguous int32 [B] tensor on the set's device")
    S = ops.check_img_size(S, exc=ValueError)
    n, H0, W0 = int(src.shape[0]), int(src.shape[1]), int(src.shape[2])
    B = idx.shape[0]
    if table.shape[0] != B:
        raise ValueError(f"augment_batch: the table has {table.shape[0]} rows, the batch {B} samples")
    if table_dev is None:
        check_table(table, H0, W0, S)
        table_dev = upload(np.ascontiguousarray(table).view(np.uint8).reshape(-1), src.device)
    if out is None:
        out = torch.empty((B, 3, S, S), dtype=torch.float32, device=src.device)
    elif out.dtype != torch.float32 or out.shape[1:] != (3, S, S) or out.shape[0] < B or not out.is_contiguous() or out.device != src.device:
        raise ValueError("augment_batch: out must be a contiguous fp32 [>=B,3,S,S] tensor on the set's device")
    m3, s3 = (L.C.c_float * 3)(*mean), (L.C.c_float * 3)(*std)
    if layers is not None:
        if layers_dev is None:
            check_ops_table(layers, B)
            layers_dev = upload(np.ascontiguousarray(layers).view(np.uint8).reshape(-1), src.device)
        nbytes = L.load().devit_augment_ops_workspace(B, S)
        ws = ops.workspace(src.device, nbytes)
        ops.call("devit_augment_batch_ops", ptr(src), n, H0, W0, ptr(idx), ptr(table_dev), ptr(layers_dev), B, S, m3, s3,
                 int(seed) & 0xFFFFFFFFFFFFFFFF, ptr(out), ptr(ws), nbytes, stream_ptr())
        return out
    nbytes = L.load().devit_augment_workspace(B, S)
    ws = ops.workspace(src.device, nbytes)
    ops.call("devit_augment_batch", ptr(src), n, H0, W0, ptr(idx), ptr(table_dev), B, S, m3, s3, int(seed) & 0xFFFFFFFFFFFFFFFF, ptr(out),
             ptr(ws), nbytes, stream_ptr())
    return out


def augment_ragged(ds, idx, table, S, mean=IMAGENET_DEFAULT_MEAN, std=IMAGENET_DEFAULT_STD, seed=0, out=None, table_dev=None, layers=None,
                   layers_dev=None, max_taps=None, force_wide=False):
    """augment_batch over a packed DeviceImageSet (devit_augment_ragged).  idx: int32 [B] on the device.  max_taps: what check_table returned
    for this table on the samples' own sizes (None: validated here, which reads idx back); force_wide: every sample through the wide kernel."""
    if not ds.ragged:
        raise ValueError("augment_ragged: the set is uniform: augment_batch(ds.images, ...)")
    L.require_device(ds.arena)
    dev = ds.arena.device
    if idx.dtype != torch.int32 or idx.dim() != 1 or idx.device != dev or not idx.is_contiguous():
        raise ValueError("augment_batch: idx must be a contiguous int32 [B] tensor on the set's device")
    S = ops.check_img_size(S, exc=ValueError)
    B = idx.shape[0]
    if table.shape[0] != B:
        raise ValueError(f"augment_batch: the table has {table.shape[0]} rows, the batch {B} samples")
    if max_taps is None:
        sizes = ds.sizes[np.clip(idx.cpu().numpy(), 0, len(ds) - 1)]
        max_taps = check_table(table, sizes[:, 0], sizes[:, 1], S)
    if table_dev is None:
        table_dev = upload(np.ascontiguousarray(table).view(np.uint8).reshape(-1), dev)
    if out is None:
        out = torch.empty((B, 3, S, S), dtype=torch.float32, device=dev)
    elif out.dtype != torch.float32 or out.shape[1:] != (3, S, S) or out.shape[0] < B or not out.is_contiguous() or out.device != dev:
        raise ValueError("augment_batch: out must be a contiguous fp32 [>=B,3,S,S] tensor on the set's device")
    if layers is not None and layers_dev is None:
        check_ops_table(layers, B)
        layers_dev = upload(np.ascontiguousarray(layers).view(np.uint8).reshape(-1), dev)
    m3, s3 = (L.C.c_float * 3)(*mean), (L.C.c_float * 3)(*std)
    nbytes = L.load().devit_augment_ragged_workspace(B, S, int(max_taps), int(layers is not None))
    ws = ops.workspace(dev, nbytes)
    ops.call("devit_augment_ragged", ptr(ds.arena), ds.arena.shape[0], ptr(ds.entries), len(ds), ptr(idx), ptr(table_dev),
             ptr(layers_dev) if layers is not None else None, B, S, m3, s3, int(seed) & 0xFFFFFFFFFFFFFFFF, ptr(out), ptr(ws), nbytes,
             int(max_taps), L.AUGMENT_FORCE_WIDE if force_wide else 0, stream_ptr())
    return out


class DeviceLoader:
    """Batches of a DeviceImageSet: (images fp32 [B,3,S,S], labels int64 [B]) device tensors, fresh per step as SyntheticLoader's and for its
    reason.  sampler: any iterable of indices with a length (RASampler, DistributedSampler, SequentialSampler); `.sampler` is what
    distill_sub.set_epoch reshuffles.  The index batch and the parameter table go up together by one pinned, non-blocking copy."""

    def __init__(self, dataset, sampler, batch_size, transform, drop_last):
        self.dataset, self.sampler, self.batch_size, self.transform, self.drop_last = dataset, sampler, int(batch_size), transform, drop_last
        if dataset.ragged:                        # a packed set: refuses it naming the images beyond the wide kernel's taps
            transform.check_set(dataset.sizes[:, 0], dataset.sizes[:, 1])
        else:
            transform.check_set(*dataset.size)    # refuses a set that needs more taps than the kernel holds

    def __len__(self):
        n = len(self.sampler)
        return n // self.batch_size if self.drop_last else (n + self.batch_size - 1) // self.batch_size

    def _batch(self, indices):
        ds, tf = self.dataset, self.transform
        B = len(indices)
        idx = np.asarray(indices, dtype=np.int32)
        if idx.min() < 0 or idx.max() >= len(ds):
            raise IndexError(f"DeviceLoader: the sampler yields indices outside 0 .. {len(ds) - 1}")
        H0, W0 = (ds.sizes[idx, 0], ds.sizes[idx, 1]) if ds.ragged else ds.size
        table, layers = tf.draw_with_ops(B, H0, W0) if getattr(tf, "has_ops", False) else (tf.draw(B, H0, W0), None)
        pad = (-idx.nbytes) % 8                   # the table's 64-bit field stays aligned behind the indices
        parts = [idx.view(np.uint8), np.zeros(pad, np.uint8), table.view(np.uint8).reshape(-1)]
        if layers is not None:
            check_ops_table(layers, B)
            parts.append(layers.view(np.uint8).reshape(-1))       # (120-byte rows: the layers' doubles stay 8-byte aligned behind them)
        both = upload(np.concatenate(parts), ds.device)
        idx_dev, at = both[:idx.nbytes].view(torch.int32), idx.nbytes + pad
        if ds.ragged:
            images = augment_ragged(ds, idx_dev, table, tf.S, tf.mean, tf.std, tf.seed, table_dev=both[at:at + table.nbytes], layers=layers,
                                    layers_dev=both[at + table.nbytes:] if layers is not None else None, max_taps=check_table(table, H0, W0, tf.S))
            return images, ds.labels.index_select(0, idx_dev.long())
        images = augment_batch(ds.images, idx_dev, table, tf.S, tf.mean, tf.std, tf.seed, table_dev=both[at:at + table.nbytes], layers=layers,
                               layers_dev=both[at + table.nbytes:] if layers is not None else None)
        return images, ds.labels.index_select(0, idx_dev.long())

    def __iter__(self):
        batch = []
        for i in self.sampler:
            batch.append(int(i))
            if len(batch) == self.batch_size:
                yield self._batch(batch)
                batch = []
        if batch and not self.drop_last:
            yield self._batch(batch)
