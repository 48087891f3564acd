"""CTC forced alignment as include/nbasr.h defines it (nbasr_ctc_forced_align), in numpy: the yardstick of the aligner's tests.

Everything runs in ``dtype`` (float32: what the kernel must give bit for bit; float64: the exact answer to hold it against).  The only
arithmetic is ``max`` and one add per cell, vectorised over the positions of the blank-extended label sequence, so 1 000 frames of
2 049 positions take about a second.  No code is shared with the package."""
import numpy as np


def forced_align(lp, length, targets, target_length, blank=0, dtype=np.float32):
    """One utterance.  lp (frames, classes); targets (ld_targets,) ints.  Returns a dict: score (``dtype`` scalar), path (frames,) int32,
    starts / ends (ld_targets,) int32, token_scores (ld_targets,) ``dtype``."""
    lp = np.asarray(lp)
    frames, classes = lp.shape
    targets = np.asarray(targets, dtype=np.int64).reshape(-1)
    ld = targets.shape[0]
    n = min(max(int(length), 0), frames)
    n_lab = min(max(int(target_length), 0), ld)
    ninf = dtype(-np.inf)
    out = dict(score=ninf, path=np.full(frames, -1, np.int32), starts=np.full(ld, -1, np.int32), ends=np.full(ld, -1, np.int32),
               token_scores=np.zeros(ld, dtype))
    labels = targets[:n_lab]
    if bool(((labels < 0) | (labels >= classes) | (labels == blank)).any()):
        out['score'] = dtype(np.nan)
        return out
    if n == 0:
        if n_lab == 0:
            out['score'] = dtype(0)
        return out
    n_pos = 2 * n_lab + 1
    ext = np.full(n_pos, blank, np.int64)
    ext[1::2] = labels
    skip = np.zeros(n_pos, bool)                                        # may s - 2 precede s?
    skip[2:] = (ext[2:] != blank) & (ext[2:] != ext[:-2])
    lp = lp[:n].astype(dtype)                                           # frames beyond the length are never touched
    v = np.full(n_pos, ninf, dtype)
    v[:2] = lp[0, ext[:2]]
    steps = np.zeros((n, n_pos), np.uint8)
    with np.errstate(invalid='ignore'):
        for t in range(1, n):
            a1 = np.concatenate(([ninf], v[:-1])).astype(dtype)
            a2 = np.where(skip, np.concatenate(([ninf, ninf], v[:-2]))[:n_pos], ninf).astype(dtype)
            m, step = v, np.zeros(n_pos, np.uint8)
            g = a1 > m                                                  # strictly greater: among equal maxima the smallest step wins
            m, step = np.where(g, a1, m), np.where(g, 1, step)
            g = a2 > m
            m, step = np.where(g, a2, m), np.where(g, 2, step)
            v = (m + lp[t, ext]).astype(dtype)
            steps[t] = step
    s = n_pos - 2 if n_pos > 1 and v[n_pos - 2] >= v[n_pos - 1] else n_pos - 1      # on a tie the path ends on the last label
    out['score'] = dtype(v[s])
    if v[s] == ninf:
        return out                                                      # no path
    where = np.empty(n, np.int64)
    for t in range(n - 1, -1, -1):
        where[t] = s
        s -= int(steps[t, s])
    out['path'][:n] = ext[where]
    for j in range(n_lab):
        at = np.nonzero(where == 2 * j + 1)[0]
        out['starts'][j], out['ends'][j] = at[0], at[-1] + 1
        total = dtype(0)
        for t in at:                                                    # increasing frame order
            total = dtype(total + lp[t, labels[j]])
        out['token_scores'][j] = total
    return out


def align_batch(log_probs, lengths, targets, target_lengths, blank=0, dtype=np.float32):
    """The kernel's outputs in its layouts: (scores (B), path (B, frames), starts, ends, token_scores (B, ld_targets))."""
    rows = [forced_align(log_probs[b], lengths[b], targets[b], target_lengths[b], blank, dtype) for b in range(len(log_probs))]
    return tuple(np.stack([r[k] for r in rows]) for k in ('score', 'path', 'starts', 'ends', 'token_scores'))


def collapse(path, blank=0):
    """The label sequence a frame-wise path spells: repeats merged, then blanks dropped (frames of -1 ignored)."""
    out, prev = [], None
    for c in path:
        c = int(c)
        if c < 0:
            continue
        if c != prev and c != blank:
            out.append(c)
        prev = c
    return out


def path_score(lp, path, dtype=np.float64):
    """(sum of lp[t][path[t]] in increasing frame order, sum of |lp[t][path[t]]| in float64) over the frames the path covers."""
    total, mag = dtype(0), 0.0
    for t, c in enumerate(path):
        if c >= 0:
            total = dtype(total + dtype(lp[t][c]))
            mag += abs(float(lp[t][c]))
    return total, mag
