"""The endpointer's definition in numpy (a helper like resample_model.py; no tests here): the sequential scan of include/nbasr.h
"endpointing" / DESIGN.md 9 "Endpoint", one frame at a time, float32 compares and integer state.  The kernel is held to it bit for bit."""
import numpy as np

STATE_WORDS = 8                  # frames, speech_frames, first_speech, last_speech, endpoint_frame, endpoint_rule, 0, 0
FRESH = (0, 0, -1, -1, -1, -1, 0, 0)
FIELDS = ('frames', 'speech_frames', 'first_speech', 'last_speech', 'endpoint_frame', 'rule')


def fresh(batch):
    return np.tile(np.array(FRESH, dtype=np.int32), (batch, 1))


def is_speech(frame, speech, margin):
    """One frame (C) float32: the two running maxima in ascending class order (a NaN is never taken), one float32 add, one compare."""
    in_s = np.zeros(frame.shape[0], dtype=bool)
    in_s[list(speech)] = True
    ms = mn = np.float32(-np.inf)
    for c in range(frame.shape[0]):
        v = np.float32(frame[c])
        if in_s[c]:
            if v > ms:
                ms = v
        elif v > mn:
            mn = v
    with np.errstate(invalid='ignore', over='ignore'):
        return bool(ms > np.float32(mn + np.float32(margin)))


def speech_mask(x, lengths, speech, margin=0.0):
    """The per-frame decision alone: x (B, n, C) float32 -> (B, n) uint8, 0 at and beyond a row's length (those frames are not read)."""
    x = np.asarray(x, dtype=np.float32)
    batch, n, _ = x.shape
    mask = np.zeros((batch, n), dtype=np.uint8)
    for b in range(batch):
        for t in range(n if lengths is None else int(lengths[b])):
            mask[b, t] = is_speech(x[b, t], speech, margin)
    return mask


def scan(mask, lengths, state, rules):
    """The integer part: the frames' decisions (B, n), lengths (B) or None, state (B, 8) int32 or None (fresh rows) -> the new state.
    ``state`` is not modified."""
    batch, n = mask.shape
    state = fresh(batch) if state is None else np.array(state, dtype=np.int32, copy=True)
    for b in range(batch):
        frames, speech_frames, first, last, ep_frame, ep_rule = (int(v) for v in state[b, :6])
        for t in range(n if lengths is None else int(lengths[b])):
            g = frames
            if mask[b, t]:
                speech_frames += 1
                last = g
                if first == -1:
                    first = g
            n_seen = g + 1
            trailing = n_seen if last == -1 else g - last
            if ep_frame == -1:
                for r, (min_speech, min_trailing, min_frames) in enumerate(rules):
                    if speech_frames >= min_speech and trailing >= min_trailing and n_seen >= min_frames:
                        ep_frame, ep_rule = g, r
                        break
            frames += 1
        state[b, :6] = (frames, speech_frames, first, last, ep_frame, ep_rule)
    return state


def step(x, lengths, state, rules, speech, margin=0.0):
    """x (B, n, C) float32, lengths (B) or None, state (B, 8) int32 or None (fresh rows) -> (new state, mask (B, n) uint8): every
    frame's decision, then the scan over them."""
    mask = speech_mask(x, lengths, speech, margin)
    return scan(mask, lengths, state, rules), mask


def fields(state):
    """{field name: (B) int32} of a state, as ``ctc.EndpointResult`` names them."""
    return {name: np.asarray(state)[:, k] for k, name in enumerate(FIELDS)}
