"""The resampler's definition in numpy (a helper like ctc_align_model.py; no tests here): band-limited sinc interpolation with a Hann
window, in absolute sample indices (DESIGN.md 9 "Resampler"; torchaudio.functional.resample's defaults):

    y[j] = sum_m x[m] (base / o) sinc(pi t) cos^2(pi t / 12),   t = (m / o - j / n) base,   base = 0.99 min(o, n)

over the integers m of [0, L) with |m n - j o| min(o, n) 99 < 600 o n, for j in [0, ceil(n L / o)).  Nothing here reads
nb_asr_amd.frontend: the support is found by testing the rule sample by sample, so the package's closed forms are checked against it.
"""
import functools
import math

import numpy as np

RATES = (8000, 11025, 22050, 32000, 44100, 48000)


def ratio(orig, new):
    g = math.gcd(orig, new)
    return orig // g, new // g


def inside(m, j, o, n):
    """The integer support rule."""
    return abs(m * n - j * o) * min(o, n) * 99 < 600 * o * n


@functools.lru_cache(maxsize=None)
def support(j, o, n):
    """(first, last) sample inside output j's support, found by walking outwards from j o / n."""
    lo = hi = (j * o) // n
    while not inside(lo, j, o, n):
        lo += 1
    while inside(lo - 1, j, o, n):
        lo -= 1
    hi = max(hi, lo)
    while inside(hi + 1, j, o, n):
        hi += 1
    return lo, hi


def time_of(m, j, o, n):
    return (m / o - j / n) * 0.99 * min(o, n)


def coefficient(m, j, o, n):
    t = time_of(m, j, o, n)
    s = 1.0 if t == 0 else math.sin(math.pi * t) / (math.pi * t)
    return (0.99 * min(o, n) / o) * s * math.cos(math.pi * t / 12.0) ** 2


def total(samples, o, n):
    return -(-n * samples // o)


def final(samples, o, n):
    """Outputs whose whole support lies below ``samples``.  A support's last sample grows with j and is at least floor(j o / n), so
    from ``total(samples)`` on none qualifies: walk down from there, one output at a time."""
    j = total(samples, o, n)
    while j > 0 and support(j - 1, o, n)[1] >= samples:
        j -= 1
    return j


def largest_support(o, n):
    return max(hi - lo + 1 for lo, hi in (support(p, o, n) for p in range(n)))


@functools.lru_cache(maxsize=None)
def phase(p, o, n):
    """(first sample, coefficients) of output p < n.  Output p + k n has the same coefficients on samples k o later: m n - j o, and
    with it t, does not change when m grows by o and j by n."""
    lo, hi = support(p, o, n)
    return lo, [coefficient(m, p, o, n) for m in range(lo, hi + 1)]


def taps_of(j, length, o, n):
    """[(sample, coefficient)] of output j in an utterance of ``length`` samples, ascending."""
    lo, row = phase(j % n, o, n)
    lo += (j // n) * o
    return [(lo + i, h) for i, h in enumerate(row) if 0 <= lo + i < length]


def resample64(x, o, n):
    """(y, bound) in float64 for one utterance x: bound[j] = sum_m |h x[m]| over the taps of y[j]."""
    x = [float(v) for v in x]
    y, bound = np.zeros(total(len(x), o, n)), np.zeros(total(len(x), o, n))
    for j in range(len(y)):
        acc = mag = 0.0
        for m, h in taps_of(j, len(x), o, n):
            acc += h * x[m]
            mag += abs(h * x[m])
        y[j], bound[j] = acc, mag
    return y, bound


def resample32(x, o, n):
    """The kernel's evaluation order in float32: the coefficient rounded once, one accumulator, taps in ascending m.  Each step is
    ``fmaf`` up to a double rounding: the product of two float32 is exact in float64, the sum is rounded to float64 and then to float32."""
    x = np.asarray(x, dtype=np.float32)
    y = np.zeros(total(len(x), o, n), dtype=np.float32)
    for j in range(len(y)):
        acc = np.float32(0)
        for m, h in taps_of(j, len(x), o, n):
            acc = np.float32(np.float64(np.float32(h)) * np.float64(x[m]) + np.float64(acc))
        y[j] = acc
    return y


def error_bound(bound, taps):
    """The float32 kernel's distance from ``resample64``, derived: one rounding per product, one per sum and one for the float32
    table, each at most 2^-24 relative to a partial sum that sum_m |h x| bounds."""
    return (taps + 2) * 2.0 ** -24 * bound
