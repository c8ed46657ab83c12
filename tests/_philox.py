"""numpy mirror of the library's dropout mask (include/devit_hip.h, "Dropout"): Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random
numbers: as easy as 1, 2, 3", SC'11; known answers from Random123's kat_vectors) and the counter layout.  Written from the header's statement,
not from the kernels: tests/test_dropout_host.py holds it to the published vectors, tests/test_gpu_dropout.py holds the kernels to it."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """ctr: four uint32 arrays (broadcastable), key: two ints -> four uint32 arrays"""
    c = [np.asarray(x, dtype=np.uint64) for x in np.broadcast_arrays(*ctr)]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]            # 32 x 32 -> 64 bits: no overflow
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & MASK, p1 >> np.uint64(32), p1 & MASK
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return [x.astype(np.uint32) for x in c]


def threshold(p):
    return min(int(np.floor(np.float64(p) * 4294967296.0)), 4294967295)


def keep_mask(seed, site, block, thr, rows, cols, pitch):
    """bool [rows][cols]: element e = row * pitch + col takes word e & 3 of counter (g lo, g hi, site, block), g = e >> 2; kept iff word >= thr"""
    assert pitch % 4 == 0 and pitch >= cols
    e = np.arange(rows, dtype=np.uint64)[:, None] * np.uint64(pitch) + np.arange(cols, dtype=np.uint64)[None, :]
    g = e >> np.uint64(2)
    w = philox4x32_10((g & MASK, g >> np.uint64(32), np.uint64(site), np.uint64(block)), (seed & 0xFFFFFFFF, seed >> 32))
    word = np.choose((e & np.uint64(3)).astype(np.int64), w)
    return word >= np.uint32(thr)
