"""The keyed bijection of csrc/r2l_perm.h and the epoch-walking sampler built on it, restated in numpy.

perm(key, n) is the bijection of [0, n) that the hard-ray pool's row choice, the ray stores' shuffles and every device sampler
use; draw_ids() is the sampler of the ray stores (on shards) and of the pixel sampler of batching mode (on pixels): draw t takes

    perm(epoch_key(seed, t // n), n)[t % n]

— a fresh permutation per epoch, without replacement inside an epoch (the InfiniteSampler of main.py:759-767), a pure function
of (seed, n, t).  These functions are the specification the tests hold the kernels to.
"""
import numpy as np

M64 = (1 << 64) - 1


def _mix(x):
    """murmur3 finalizer on uint32 arrays (wrapping arithmetic)."""
    x = x.astype(np.uint32, copy=True)
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x85ebca6b)
    x ^= x >> np.uint32(13)
    x *= np.uint32(0xc2b2ae35)
    x ^= x >> np.uint32(16)
    return x


def _mix1(x):
    return int(_mix(np.array([x & 0xffffffff], dtype=np.uint32))[0])


def round_keys(key):
    key = int(key) & M64
    lo, hi = key & 0xffffffff, key >> 32
    return [_mix1(lo), _mix1(hi ^ 0x9e3779b9), _mix1(lo ^ 0x7f4a7c15), _mix1((hi + 0x6a09e667) & 0xffffffff)]


def half_bits(n):
    bits = 2
    while (1 << bits) < n:
        bits += 2
    return bits // 2


def _feistel(x, hb, k):
    mask = np.uint32((1 << hb) - 1)
    l = (x >> np.uint64(hb)).astype(np.uint32) & mask
    r = x.astype(np.uint32) & mask
    for i in range(4):
        f = _mix(r ^ np.uint32(k[i])) & mask
        l, r = r, l ^ f
    return (l.astype(np.uint64) << np.uint64(hb)) | r.astype(np.uint64)


def perm_at(key, n, idx):
    """pi(key, n) evaluated at the indices idx (each < n): int64 array."""
    hb, k = half_bits(n), round_keys(key)
    x = _feistel(np.asarray(idx, dtype=np.uint64), hb, k)
    while True:
        out = np.nonzero(x >= np.uint64(n))[0]
        if out.size == 0:
            return x.astype(np.int64)
        x[out] = _feistel(x[out], hb, k)  # cycle walking


def perm(key, n):
    """The bijection of [0, n) that r2l_pool_pick(n, n, key) writes and r2l_store_append shuffles by: int64[n]."""
    return perm_at(key, n, np.arange(n, dtype=np.uint64))


def epoch_key(seed, epoch):
    """splitmix64 finalizer of seed + (epoch + 1) * 0x9E3779B97F4A7C15 (mod 2^64)."""
    z = (int(seed) + (int(epoch) + 1) * 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def draw_ids(seed, n, draw0, n_draw):
    """Ids in [0, n) of the draws draw0 .. draw0 + n_draw - 1: int64[n_draw], perm(epoch_key(seed, t // n), n)[t % n] for each t."""
    out = np.empty(n_draw, dtype=np.int64)
    t, j = int(draw0), 0
    while j < n_draw:
        e, r = divmod(t, n)
        m = min(n - r, n_draw - j)
        out[j:j + m] = perm_at(epoch_key(seed, e), n, np.arange(r, r + m, dtype=np.uint64))
        t, j = t + m, j + m
    return out
