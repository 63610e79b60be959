"""Integer model of the mini-batch draw of csrc/batch.hip / pinn_batch_draw (TEST INFRASTRUCTURE; pure numpy).

For batch slot j in [0, B): lo = floor(j N / B), hi = floor((j + 1) N / B), r = word 0 of Philox4x32-10 with counter
(j_lo32, j_hi32, t_lo32, t_hi32) and key (seed_lo32, rank), idx_j = lo + ((r (hi - lo)) >> 32)."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """The four output words of Philox4x32-10 (Salmon et al. 2011).  counter: 4 words, key: 2 words; each a Python
    int or a uint64 numpy array holding 32-bit values (arrays broadcast)."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & np.uint64(MASK) for c in counter)
    k0, k1 = (np.asarray(k, dtype=np.uint64) & np.uint64(MASK) for k in key)
    m32, s32 = np.uint64(MASK), np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2         # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & m32, (p0 >> s32) ^ c3 ^ k1, p0 & m32
        k0, k1 = (k0 + np.uint64(W0)) & m32, (k1 + np.uint64(W1)) & m32
    return c0, c1, c2, c3


def strata(n, b):
    """(lo, hi) int64 arrays of the b strata of n store points."""
    j = np.arange(int(b), dtype=np.int64)
    return j * int(n) // int(b), (j + 1) * int(n) // int(b)


def draw(n, b, t, seed=0, rank=0):
    """int64 store indices [b] of draw number t."""
    n, b, t = int(n), int(b), int(t)
    if not 1 <= b <= n:
        raise ValueError("need 1 <= b <= n")
    lo, hi = strata(n, b)
    j = np.arange(b, dtype=np.uint64)
    r = philox4x32_10((j & np.uint64(MASK), j >> np.uint64(32), t & MASK, (t >> 32) & MASK),
                      (int(seed) & MASK, int(rank) & MASK))[0]
    return lo + ((r * (hi - lo).astype(np.uint64)) >> np.uint64(32)).astype(np.int64)
