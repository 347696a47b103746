"""An independent statement of the dropout generator, numpy only (nothing of the library is imported here).

Philox4x32-10 as published (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11; the Random123
library's philox4x32 with ten rounds): a 128-bit counter (c0, c1, c2, c3) and a 64-bit key (k0, k1).  One round is

    hi0:lo0 = 0xD2511F53 * c0        hi1:lo1 = 0xCD9E8D57 * c2            (32 x 32 -> 64 bit products)
    (c0, c1, c2, c3) <- (hi1 ^ c1 ^ k0,  lo1,  hi0 ^ c3 ^ k1,  lo0)

and the key is bumped by (0x9E3779B9, 0xBB67AE85) between rounds.  tests/test_philox_ref.py checks the known-answer vectors.

The dropout stream built on it: the draws of elements [4q, 4q + 4) of a tensor are the four outputs of counter
(q lo, q hi, offset lo, offset hi) under key (seed lo, seed hi); an element is kept iff its draw >= floor(float32(p) * 2^32), clamped to
2^32 - 1; kept elements are scaled by float32(1) / (float32(1) - float32(p)).
"""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = 0xFFFFFFFF


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Vectorised over uint64 arrays (or scalars) holding 32-bit words; returns the four output words as uint64 arrays."""
    c0, c1, c2, c3, k0, k1 = (np.asarray(v, dtype=np.uint64) & np.uint64(MASK32) for v in (c0, c1, c2, c3, k0, k1))
    m32, s32 = np.uint64(MASK32), np.uint64(32)
    for _ in range(10):
        p0 = np.uint64(M0) * c0          # both factors below 2^32: the product fits 64 bits
        p1 = np.uint64(M1) * c2
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & m32, (p0 >> s32) ^ c3 ^ k1, p0 & m32
        k0 = (k0 + np.uint64(W0)) & m32
        k1 = (k1 + np.uint64(W1)) & m32
    return c0, c1, c2, c3


def threshold(p):
    """floor(float32(p) * 2^32), clamped to [0, 2^32 - 1] (float32 -> float64 is exact, and so is the product with a power of two)."""
    t = int(np.floor(float(np.float32(p)) * 4294967296.0))
    return min(max(t, 0), MASK32)


def keep_scale(p):
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


def keep_mask(n, p, seed, offset):
    """(draws, keep): the n 32-bit draws (uint32) and the keep booleans of an n-element tensor at stream position ``offset``."""
    seed, offset = int(seed) & 0xFFFFFFFFFFFFFFFF, int(offset) & 0xFFFFFFFFFFFFFFFF
    q = np.arange((n + 3) // 4, dtype=np.uint64)
    r = philox4x32_10(q & np.uint64(MASK32), q >> np.uint64(32), offset & MASK32, offset >> 32, seed & MASK32, seed >> 32)
    draws = np.stack(r, axis=1).reshape(-1)[:n].astype(np.uint32)
    return draws, draws >= np.uint32(threshold(p))
