"""The keyword spotter's definition in numpy (a helper like endpoint_model.py; no tests here): include/nbasr.h "keywords" / DESIGN.md 9
"Keywords", one frame at a time, float32 compares, one float32 subtract and one float32 add per state.  The kernel is held to it bit for
bit, NaN behaviour included."""
import numpy as np

STATE_WORDS = 136                # frames, hit (frame, start, score), best (frame, start, score), 0, V[64], start[64]
MAX_STATES = 64
INT_FIELDS = {'frames': 0, 'hit_frame': 1, 'hit_start': 2, 'best_frame': 4, 'best_start': 5}
FLOAT_FIELDS = {'hit_score': 3, 'best_score': 6}
NEG_INF = np.float32(-np.inf)
NEG_INF_BITS = int(np.array(-np.inf, dtype=np.float32).view(np.int32))


def fresh(batch, n_keywords):
    """(B, K, 136) int32: (0, -1, -1, -inf, -1, -1, -inf, 0), V = -inf, start = -1."""
    row = np.full(STATE_WORDS, -1, dtype=np.int32)
    row[0] = row[7] = 0
    row[3] = row[6] = NEG_INF_BITS
    row[8:8 + MAX_STATES] = NEG_INF_BITS
    return np.tile(row, (batch, n_keywords, 1))


def states_of(keyword, blank):
    """z(s) for the S = 2 L - 1 states: token, blank, token, ..., token."""
    keyword = [int(t) for t in keyword if int(t) >= 0]               # (a row of the (K, 32) table ends in -1s)
    z = []
    for i, t in enumerate(keyword):
        if i:
            z.append(int(blank))
        z.append(t)
    return z


def frame_max(frame):
    m = NEG_INF
    for c in range(frame.shape[0]):
        v = np.float32(frame[c])
        if v > m:                                                     # a NaN is never taken
            m = v
    return m


def step(x, lengths, state, tokens, thresholds, blank):
    """x (B, n, C) float32, lengths (B) or None, state (B, K, 136) int32 or None (fresh rows), tokens: K token sequences (or the (K, 32)
    table), thresholds (K) -> (new state, scores (B, K, n) float32, starts (B, K, n) int32); -inf and -1 at and beyond a row's length.
    ``state`` is not modified."""
    x = np.asarray(x, dtype=np.float32)
    batch, n, _ = x.shape
    n_keywords = len(tokens)
    state = fresh(batch, n_keywords) if state is None else np.array(state, dtype=np.int32, copy=True)
    scores = np.full((batch, n_keywords, n), NEG_INF, dtype=np.float32)
    starts = np.full((batch, n_keywords, n), -1, dtype=np.int32)
    with np.errstate(invalid='ignore', over='ignore'):
        for b in range(batch):
            rows = n if lengths is None else int(lengths[b])
            maxima = [frame_max(x[b, t]) for t in range(rows)]
            for k in range(n_keywords):
                z = states_of(tokens[k], blank)
                S = len(z)
                threshold = np.float32(thresholds[k])
                row = state[b, k]
                g, hit_frame, hit_start, best_frame, best_start = (int(row[w]) for w in (0, 1, 2, 4, 5))
                hit_score, best_score = row[3:4].view(np.float32)[0], row[6:7].view(np.float32)[0]
                V = row[8:8 + MAX_STATES].view(np.float32).copy()
                start = row[8 + MAX_STATES:].copy()
                za = np.array(z)
                advance = np.arange(S) >= 1
                skip = np.array([s % 2 == 0 and s >= 2 and z[s] != z[s - 2] for s in range(S)])
                for t in range(rows):                                 # every state at once: all reads are of the previous frame's values
                    pV, ps = V[:S], start[:S]
                    best, src = np.full(S, NEG_INF), np.full(S, -1, dtype=np.int32)
                    for allowed, shift in ((True, 0), (advance, 1), (skip, 2)):     # stay, advance, skip the blank: in this order
                        cV = np.concatenate([np.full(shift, NEG_INF), pV[:max(S - shift, 0)]])[:S]
                        cs = np.concatenate([np.full(shift, -1, dtype=np.int32), ps[:max(S - shift, 0)]])[:S]
                        take = allowed & (cV > best)
                        best, src = np.where(take, cV, best), np.where(take, cs, src)
                    if np.float32(0.0) > best[0]:                     # state 0 only: a fresh start at this frame
                        best[0], src[0] = 0.0, g
                    d = (x[b, t, za] - maxima[t]).astype(np.float32)  # one float32 subtract
                    V[:S], start[:S] = (best + d).astype(np.float32), src            # one float32 add
                    score, src = V[S - 1], int(start[S - 1])
                    if score > best_score:
                        best_score, best_frame, best_start = score, g, src
                    if hit_frame == -1 and score >= threshold:
                        hit_frame, hit_start, hit_score = g, src, score
                    scores[b, k, t], starts[b, k, t] = score, src
                    g += 1
                row[0], row[1], row[2], row[4], row[5], row[7] = g, hit_frame, hit_start, best_frame, best_start, 0
                row[3:4].view(np.float32)[0], row[6:7].view(np.float32)[0] = hit_score, best_score
                row[8:8 + MAX_STATES] = V.view(np.int32)
                row[8 + MAX_STATES:] = start
    return state, scores, starts


def fields(state):
    """{field name: (B, K)} of a state, as ``ctc.KeywordResult`` names them: int32, the two scores float32."""
    state = np.ascontiguousarray(np.asarray(state, dtype=np.int32))
    out = {name: state[:, :, w] for name, w in INT_FIELDS.items()}
    out.update({name: state.view(np.float32)[:, :, w] for name, w in FLOAT_FIELDS.items()})
    return out
