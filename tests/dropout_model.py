"""Counter-based dropout's definition in numpy (include/nbasr.h "dropout"; a helper like confidence_model.py, no tests here).

The mask of an element is a pure function of (seed, call, row, frame): Philox4x32-10 keyed by the seed, counted by the element's group of
four frames and the call.  Nothing is stored; forward and backward compute the same words.  Every step below is integer arithmetic or one
float32 multiply / add, so the device is compared with ``apply`` bit for bit.

  philox4x32_10(counter, key)      the generator: (..., 4) uint32 counters, a (2,) key -> (..., 4) uint32 words
  words(rows, frames, seed, call, row0)
                                   the word of each element of a rows x frames tensor (the row pitch does not enter)
  thr(p), scale(p)                 the keep rule: an element is kept iff its word >= thr(p); kept elements are multiplied by scale(p)
  multiplier(...)                  scale where kept, 0 where dropped, as float32
  apply(x, p, seed, call, row0, skips)
                                   y = x * multiplier, then the node's sum over up to three skips, left to right
"""
import numpy as np

MASK32 = 0xFFFFFFFF
MASK64 = 0xFFFFFFFFFFFFFFFF
M0, M1 = 0xD2511F53, 0xCD9E8D57          # the round multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85          # the Weyl constants added to the key between rounds
ROUNDS = 10


def philox4x32_10(counter, key):
    """Philox4x32 with ten rounds (Salmon et al., SC'11).  ``counter``: (..., 4) uint32, ``key``: two 32-bit words."""
    c = [np.asarray(counter)[..., i].astype(np.uint64) for i in range(4)]
    k0, k1 = int(key[0]) & MASK32, int(key[1]) & MASK32
    for rnd in range(ROUNDS):
        if rnd:
            k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]          # 32 x 32 -> 64 bits: no overflow in uint64
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & np.uint64(MASK32), p1 >> np.uint64(32), p1 & np.uint64(MASK32)
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
    return np.stack(c, axis=-1).astype(np.uint32)


def _halves(v):
    """A 64-bit pattern (a negative int is its two's complement) as (low, high) 32-bit words."""
    v = int(v) & MASK64
    return v & MASK32, v >> 32


def groups_per_row(frames):
    return (frames + 3) // 4


def words(rows, frames, seed, call, row0=0):
    """(rows, frames) uint32: element (r, t) takes word t & 3 of philox(counter = (g_lo, g_hi, call_lo, call_hi), key = (seed_lo, seed_hi)),
    g = (row0 + r) * ceil(frames / 4) + (t >> 2) as a 64-bit number (modulo 2^64)."""
    gpr = groups_per_row(frames)
    out = np.zeros((rows, frames), dtype=np.uint32)
    if rows == 0 or frames == 0:
        return out
    row = np.full(rows, int(row0) & MASK64, dtype=np.uint64) + np.arange(rows, dtype=np.uint64)
    g = row[:, None] * np.uint64(gpr) + np.arange(gpr, dtype=np.uint64)[None, :]          # uint64 arrays wrap modulo 2^64
    call_lo, call_hi = _halves(call)
    counter = np.empty((rows, gpr, 4), dtype=np.uint32)
    counter[..., 0] = (g & np.uint64(MASK32)).astype(np.uint32)
    counter[..., 1] = (g >> np.uint64(32)).astype(np.uint32)
    counter[..., 2] = call_lo
    counter[..., 3] = call_hi
    return philox4x32_10(counter, _halves(seed)).reshape(rows, gpr * 4)[:, :frames]


def thr(p):
    """floor(p 2^32 + 0.5) in double precision, an integer in [0, 2^32]."""
    p = float(p)
    if not 0.0 <= p <= 1.0:
        raise ValueError(f'p={p} is outside [0, 1]')
    return int(np.floor(p * 4294967296.0 + 0.5))


def scale(p):
    """(float)(1 / (1 - p)), and 0 for p = 1."""
    p = float(p)
    return np.float32(0.0) if p == 1.0 else np.float32(1.0 / (1.0 - p))


def kept(rows, frames, p, seed, call, row0=0):
    """(rows, frames) bool: word >= thr as unsigned 64-bit values."""
    return words(rows, frames, seed, call, row0).astype(np.uint64) >= np.uint64(thr(p))


def multiplier(rows, frames, p, seed, call, row0=0):
    return np.where(kept(rows, frames, p, seed, call, row0), scale(p), np.float32(0.0)).astype(np.float32)


def apply(x, p, seed, call, row0=0, skips=()):
    """x (rows, frames) float32 -> x * (kept ? scale : 0) in float32: a dropped Inf or NaN gives NaN, as a multiply does.  With skips, the
    node's sum as the skip-sum kernel forms it with the dropped tensor as its first term: from +0, left to right,
    (((0 + drop(x)) + skip0) + skip1) + skip2 -- equal to ((drop(x) + skip0) + skip1) + skip2 but for the sign of a zero."""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(all='ignore'):
        y = x * multiplier(x.shape[0], x.shape[1], p, seed, call, row0)
        if skips:
            y = np.float32(0.0) + y
            for s in skips:
                y = y + np.asarray(s, dtype=np.float32)
    return y.astype(np.float32)
