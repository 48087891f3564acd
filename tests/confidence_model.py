"""The confidence estimator's definition in numpy (include/nbasr.h "confidence"; a helper like segment_model.py, no tests here).

Steps 1 and 2 -- the label and the frame confidence -- run in float64 (the yardstick) or float32, each frame from its own C values alone;
step 3 quantises; steps 4 to 6 -- tokens, the 16-word record, the floats -- are integers, walked one frame after the other.  ``step``
takes a chunk and the record of the chunks before it, so any chunking can be replayed; ``path=`` gives the labels of a hypothesis.

``tolerance`` is the bound on |q_device - q_float64|, derived below from the operation count of step 2.  ``assert_q_close`` is the one
comparison helper the tests use: it is handed the q of whatever is under test and compares with the float64 model.
"""
import math

import numpy as np

ONE = 1 << 24
STATE_WORDS, TOKEN_WORDS = 16, 8
MEASURES = ('prob', 'entropy', 'tsallis')
FIELDS = ('frames', 'prev_label', 'open_start', 'open_min_q', 'open_sum_lo', 'open_sum_hi', 'tokens', 'utt_min_q', 'utt_sum_lo', 'utt_sum_hi',
          'utt_frames', 'bad')
FRESH = [0, -1, -1, ONE, 0, 0, 0, ONE, 0, 0, 0, 0, 0, 0, 0, 0]
CAP = 4096                       # units of 2^-24: 2^-12, the most a bound may be for a test's inputs (a wrong normaliser or log base is far beyond)


def fresh(batch):
    return np.array([FRESH] * batch, dtype=np.int32).reshape(batch, STATE_WORDS)


# ---- steps 1 to 3: one frame ---------------------------------------------------------------------------------------------------------
def greedy_labels(x):
    """The smallest index among the largest values of each frame: (..., C) -> (...) (np.argmax takes the first maximum)."""
    return np.argmax(x, axis=-1).astype(np.int64)


def tsallis_k(classes, alpha):
    """k = C^(1 - alpha) in double precision, alpha the float32 value the step is handed."""
    return float(classes) ** (1.0 - float(np.float32(alpha)))


def frame_confidence(x, labels, measure, alpha=1 / 3, dtype=np.float64, log=np.log):
    """Step 2 for the frames x (..., C), each on its own: the confidence in [0, 1] as ``dtype``.  ``log``: the logarithm (np.log; a test
    hands np.log2 to show that the comparison helper notices)."""
    x = np.asarray(x).astype(dtype)
    classes = x.shape[-1]
    with np.errstate(all='ignore'):
        m = x.max(axis=-1, keepdims=True)
        s = np.exp(x - m).sum(axis=-1, keepdims=True, dtype=dtype)
        lp = x - (m + log(s))
        if measure == 'prob':
            conf = np.exp(np.take_along_axis(lp, np.asarray(labels)[..., None], axis=-1))[..., 0]
        elif measure == 'entropy':
            p = np.exp(lp)
            conf = 1 + np.where(p != 0, p * lp, 0).sum(axis=-1, dtype=dtype) / log(dtype(classes))
        elif measure == 'tsallis':
            k = dtype(tsallis_k(classes, alpha))
            t = np.exp(dtype(np.float32(alpha)) * lp).sum(axis=-1, dtype=dtype)          # exp(-inf) = 0
            conf = (k - t) / (k - 1)
        else:
            raise ValueError(measure)
        return np.where(conf > 0, np.minimum(conf, 1), 0).astype(dtype)                  # clamped; a NaN becomes 0


def quantise(conf):
    """Step 3: rint(conf * 2^24), an integer in [0, 2^24]."""
    return np.rint(np.asarray(conf, dtype=np.float64) * ONE).astype(np.int64)


def frames_q(x, measure, alpha=1 / 3, blank=0, path=None, dtype=np.float64, log=np.log):
    """(labels, q, bad) of x (B, n, C): steps 1 to 3 of every frame.  ``path`` (B, n): the labels instead of the greedy ones; one outside
    [0, C) counts as blank and is reported in ``bad`` (B, n) bool."""
    x = np.asarray(x, dtype=np.float32)
    if path is None:
        labels, bad = greedy_labels(x), np.zeros(x.shape[:2], dtype=bool)
    else:
        path = np.asarray(path).astype(np.int64)
        bad = (path < 0) | (path >= x.shape[-1])
        labels = np.where(bad, blank, path)
    return labels, quantise(frame_confidence(x, labels, measure, alpha, dtype, log)), bad


# ---- steps 4 to 6: integers ----------------------------------------------------------------------------------------------------------
def join(lo, hi):
    return (int(hi) << 32) | (int(lo) & 0xFFFFFFFF)


def split(value):
    lo, hi = value & 0xFFFFFFFF, value >> 32
    return (lo - (1 << 32) if lo >> 31 else lo), hi


def scan(labels, q, lengths, state, blank, final, bad=None):
    """The tokens of one step.  labels, q (B, n) integers; lengths (B) or None; state (B, 16) int32 or None (fresh rows).
    -> (state_out (B, 16) int32, table (B, n + 1, 8) int32 filled with -1 past the count, counts (B) int32)."""
    batch, n = labels.shape
    state = fresh(batch) if state is None else np.array(state, dtype=np.int32)
    table = np.full((batch, n + 1, TOKEN_WORDS), -1, dtype=np.int32)
    counts = np.zeros(batch, dtype=np.int32)
    for b in range(batch):
        frames, prev, open_start, open_min = (int(v) for v in state[b, :4])
        open_sum, tokens, utt_min = join(state[b, 4], state[b, 5]), int(state[b, 6]), int(state[b, 7])
        utt_sum, utt_frames, was_bad = join(state[b, 8], state[b, 9]), int(state[b, 10]), int(state[b, 11])
        closed = []

        def close(end):
            closed.append((prev, open_start, end, open_min, *split(open_sum), 0, 0))

        length = n if lengths is None else min(max(int(lengths[b]), 0), n)
        for t in range(length):
            label, qt = int(labels[b, t]), int(q[b, t])
            if open_start >= 0 and label != prev:                # the first frame that does not continue the open token closes it
                close(frames)
                open_start = -1
            if label != blank:
                if open_start < 0:
                    open_start, open_min, open_sum = frames, ONE, 0
                open_min, open_sum = min(open_min, qt), open_sum + qt
                utt_min, utt_sum, utt_frames = min(utt_min, qt), utt_sum + qt, utt_frames + 1
            prev = label
            frames += 1
            if bad is not None and bad[b, t]:
                was_bad = 1
        if final:
            if open_start >= 0:
                close(frames)
            prev, open_start = -1, -1
        if open_start < 0:
            open_min, open_sum = ONE, 0
        for k, entry in enumerate(closed):
            table[b, k] = entry
        counts[b] = len(closed)
        state[b] = [frames, prev, open_start, open_min, *split(open_sum), tokens + len(closed), utt_min, *split(utt_sum), utt_frames, was_bad,
                    0, 0, 0, 0]
    return state, table, counts


def step(x, lengths, state, measure, alpha=1 / 3, blank=0, final=False, path=None, dtype=np.float64):
    """One step over the chunk x (B, n, C) -> (state_out, table, counts, frame_q (B, n) int32 with -1 at and beyond a row's length)."""
    x = np.asarray(x, dtype=np.float32)
    batch, n = x.shape[:2]
    if n:
        labels, q, bad = frames_q(x, measure, alpha, blank, path, dtype)
    else:
        labels = q = np.zeros((batch, 0), dtype=np.int64)
        bad = np.zeros((batch, 0), dtype=bool)
    out = scan(labels, q, lengths, state, blank, final, bad)
    within = np.arange(n)[None, :] < (np.full(batch, n) if lengths is None else np.clip(np.asarray(lengths), 0, n))[:, None]
    return (*out, np.where(within, q, -1).astype(np.int32))


def tokens_of(table, counts):
    """Per row [(label, start, end, min_q, sum_q)] of a step's table."""
    return [[(int(e[0]), int(e[1]), int(e[2]), int(e[3]), join(e[4], e[5])) for e in table[b, :int(counts[b])]] for b in range(len(counts))]


def mean_of(sum_q, frames):
    """Step 6: float32(double(sum_q) / (double(frames) * 2^24))."""
    return np.float32(np.float64(sum_q) / (np.float64(frames) * np.float64(ONE)))


def min_of(min_q):
    """Step 6: float32(min_q) * 2^-24."""
    return np.float32(min_q) * np.float32(2.0 ** -24)


# ---- the bound on q --------------------------------------------------------------------------------------------------------------------
# Units of u = 2^-24, which is also float32's unit roundoff: one rounding of a value v costs at most |v| units.  E is the documented
# error of the library's expf and logf in ulps; an ulp is 2 u relative, so one call costs 2 E units relative.  The HIP device library
# documents 1 ulp for both; E = 3 is what OpenCL's full profile allows a conforming exp and log, and covers numpy's float32 too.
# With C classes, M = the frame's largest finite |x|, L = ln C, and d_c = x_c - m <= 0:
#   s   = sum exp(d_c):  each d_c is rounded (|d_c| units absolute, which exp turns into |d_c| exp(d_c) <= 1/e < 0.37), each exp costs 2 E
#         relative, the C - 1 additions of positive terms at most C - 1 relative in all; s >= 1, so relative to s at most 2 E + 1.37 C;
#   lse = m + log(s):    log turns that relative error into an absolute one and adds 2 E L of its own; the addition rounds a value of at
#         most M + L:    A_lse = (2 E + 1.37 C) + 2 E L + (M + L);
#   lp_c = x_c - lse:    one rounding of a value of at most 2 M + L -- the cancellation that grows with |x|:  A_lp = A_lse + 2 M + L;
#   prob:     exp turns A_lp into a relative error of p <= 1 and adds 2 E:                                    A_lp + 2 E;
#   entropy:  the terms p_c lp_c carry p_c |lp_c| (A_lp + 2 E + 1) + p_c A_lp, their sum over c is at most H (A_lp + 2 E + 1) + A_lp with
#             H = -sum p lp <= L; adding C terms of one sign costs (C - 1) H more; dividing by the rounded L and adding 1 costs 3; over L:
#                                                                                                  (A_lp + 2 E + C) + A_lp / L + 3;
#   tsallis:  alpha lp_c is rounded (< 0.37 after exp, as above), exp(alpha lp_c) carries alpha A_lp + 2 E relative, the sum T <= k adds
#             (C - 1) T, k itself is a rounded double and k - T rounds once more; divided by k - 1, plus the division's own rounding:
#                                                              (k (alpha A_lp + 2 E + C + 2) + 0.37 C) / (k - 1) + 1;
# and one unit more for the two quantisations (half a unit each).  The bound grows with M and, for tsallis, as alpha approaches 1.
ULPS = 3


def tolerance(classes, max_abs, measure, alpha=1 / 3):
    """The most |q - q_float64| may be for a frame of ``classes`` values of magnitude up to ``max_abs``, in units of 2^-24."""
    c, m, e, ln_c = float(classes), float(max_abs), float(ULPS), math.log(classes)
    a_lse = (2 * e + 1.37 * c) + 2 * e * ln_c + (m + ln_c)
    a_lp = a_lse + 2 * m + ln_c
    if measure == 'prob':
        bound = a_lp + 2 * e
    elif measure == 'entropy':
        bound = (a_lp + 2 * e + c) + a_lp / ln_c + 3
    else:
        k = tsallis_k(classes, alpha)
        bound = (k * (float(alpha) * a_lp + 2 * e + c + 2) + 0.37 * c) / (k - 1) + 1
    return int(math.ceil(bound)) + 1


def assert_q_close(got_q, x, lengths, measure, alpha=1 / 3, blank=0, path=None):
    """|got_q - q of the float64 model| <= tolerance(C, the frame's largest finite |x|) at every frame within the lengths, and the bound
    itself within CAP.  -> the largest deviation seen, in units of 2^-24."""
    x = np.asarray(x, dtype=np.float32)
    batch, n, classes = x.shape
    if n == 0:
        return 0
    _, want, _ = frames_q(x, measure, alpha, blank, path)
    within = np.arange(n)[None, :] < (np.full(batch, n) if lengths is None else np.clip(np.asarray(lengths), 0, n))[:, None]
    finite = np.where(np.isfinite(x), np.abs(x), 0).max(axis=-1)
    worst = 0
    for b, t in zip(*np.nonzero(within)):
        bound = tolerance(classes, finite[b, t], measure, alpha)
        assert bound <= CAP, (bound, classes, finite[b, t], measure)
        off = abs(int(got_q[b, t]) - int(want[b, t]))
        assert off <= bound, (b, t, measure, int(got_q[b, t]), int(want[b, t]), bound)
        worst = max(worst, off)
    return worst
