"""Referee of the native dropout (gsn_amd/dropout.py, csrc/dropout_core.h): Philox4x32-10 in numpy with uint64 arithmetic, the mask of one
call, and forward / backward in float32 with a separately rounded multiply and add.  Written from the statement of the stream (DESIGN.md
8d), not from the kernel: group q = e >> 2, counter = (lo32 q, hi32 q, lo32 calls, hi32 calls), key = (lo32 seed, hi32 seed), word e & 3,
keep iff word >= threshold(p)."""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
LO = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


def philox4x32_10(counter, key):
    """counter: four uint64 arrays (or scalars) of 32-bit values, key: two -> four uint64 arrays of 32-bit words."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & LO for c in counter)
    k0, k1 = (np.asarray(k, dtype=np.uint64) & LO for k in key)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2                     # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> S32) ^ c1 ^ k0, p1 & LO, (p0 >> S32) ^ c3 ^ k1, p0 & LO
        k0, k1 = (k0 + W0) & LO, (k1 + W1) & LO
    return c0, c1, c2, c3


def threshold(p):
    return min(2 ** 32 - 1, int(round(float(p) * 2.0 ** 32)))


def scale(p):
    return np.float32(1.0 / (1.0 - float(p)))          # the double division, rounded once


def _u64(v):
    return np.uint64(int(v) & (2 ** 64 - 1))


def keep_at(seed, calls, e, thr):
    """keep decision of single elements: e an array of element numbers (uint64 range)"""
    e = np.asarray(e, dtype=np.uint64)
    seed, calls = _u64(seed), _u64(calls)
    q = e >> np.uint64(2)
    words = philox4x32_10((q & LO, q >> S32, calls & LO, calls >> S32), (seed & LO, seed >> S32))
    lane = (e & np.uint64(3)).astype(np.int64)
    w = np.choose(lane, [np.broadcast_to(x, e.shape) for x in words])
    return w >= np.uint64(thr)


def mask(seed, calls, n, thr):
    """bool [n]: the kept elements of call (seed, calls) on a tensor of n elements"""
    if n == 0:
        return np.zeros(0, dtype=bool)
    seed, calls = _u64(seed), _u64(calls)
    q = np.arange((n + 3) // 4, dtype=np.uint64)
    words = philox4x32_10((q & LO, q >> S32, calls & LO, calls >> S32), (seed & LO, seed >> S32))
    return (np.stack(words, 1).reshape(-1)[:n] >= np.uint64(thr))


def forward(x, res, seed, calls, p):
    """float32 array of x's shape: res + (keep ? x * scale : +0), product and sum rounded separately"""
    x = np.asarray(x, dtype=np.float32)
    keep = mask(seed, calls, x.size, threshold(p)).reshape(x.shape)
    with np.errstate(all="ignore"):
        v = np.where(keep, (x * scale(p)).astype(np.float32), np.float32(0.0))
        return v if res is None else (np.asarray(res, dtype=np.float32) + v).astype(np.float32)


def backward(g, seed, calls, p):
    g = np.asarray(g, dtype=np.float32)
    keep = mask(seed, calls, g.size, threshold(p)).reshape(g.shape)
    with np.errstate(all="ignore"):
        return np.where(keep, (g * scale(p)).astype(np.float32), np.float32(0.0))
