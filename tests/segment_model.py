"""The segmenter's definition in numpy (a helper like endpoint_model.py; no tests here): the automaton of include/nbasr.h "segmentation" /
DESIGN.md 9 "Segments", one frame at a time, on the endpointer's speech decision (endpoint_model.speech_mask) and integer state.  The
kernel is held to it bit for bit."""
import numpy as np

from endpoint_model import speech_mask

HEAD_WORDS = 8                   # frames, speech_run, silence_run, open_start, count, 0, 0, 0
ENTRY_WORDS = 4                  # start, end, reason, 0
FRESH_HEAD = (0, 0, 0, -1, 0, 0, 0, 0)
FRESH_ENTRY = (-1, -1, -1, 0)
FIELDS = ('frames', 'speech_run', 'silence_run', 'open_start', 'count')


def state_words(capacity):
    return HEAD_WORDS + ENTRY_WORDS * capacity


def fresh(batch, capacity):
    return np.tile(np.array(FRESH_HEAD + FRESH_ENTRY * capacity, dtype=np.int32), (batch, 1))


def scan(mask, lengths, state, min_speech, min_silence, max_frames, capacity):
    """The integer part: the frames' decisions (B, n), lengths (B) or None, state (B, 8 + 4 S) int32 or None (fresh rows) -> the new
    state.  ``state`` is not modified."""
    batch, n = mask.shape
    state = fresh(batch, capacity) if state is None else np.array(state, dtype=np.int32, copy=True)
    assert state.shape == (batch, state_words(capacity))
    for b in range(batch):
        frames, speech_run, silence_run, open_start, count = (int(v) for v in state[b, :5])
        for t in range(n if lengths is None else int(lengths[b])):
            g, s = frames, bool(mask[b, t])
            if s:
                speech_run, silence_run = speech_run + 1, 0
            else:
                silence_run, speech_run = silence_run + 1, 0
            closed = None
            if open_start == -1 and s and speech_run >= min_speech:
                open_start = g - min_speech + 1
            elif open_start != -1 and not s and silence_run >= min_silence:
                closed = (open_start, g - silence_run + 1, 0, 0)
            elif open_start != -1 and max_frames and g + 1 - open_start >= max_frames:
                closed = (open_start, g + 1, 1, 0)
                speech_run = silence_run = 0
            if closed is not None:
                at = HEAD_WORDS + ENTRY_WORDS * (count % capacity)
                state[b, at:at + ENTRY_WORDS] = closed
                count, open_start = count + 1, -1
            frames = g + 1
        state[b, :5] = (frames, speech_run, silence_run, open_start, count)
    return state


def step(x, lengths, state, rules, speech, margin=0.0):
    """x (B, n, C) float32, lengths (B) or None, state or None (fresh rows), rules = (min_speech, min_silence, max_frames, capacity) ->
    (new state, mask (B, n) uint8): every frame's decision, then the scan over them."""
    mask = speech_mask(x, lengths, speech, margin)
    return scan(mask, lengths, state, *rules), mask


def ring(state):
    """(B, S, 4) of a state."""
    state = np.asarray(state)
    return state[:, HEAD_WORDS:].reshape(state.shape[0], -1, ENTRY_WORDS)


def spans(state, include_open=False):
    """Per row the last min(count, S) closed segments (start, end, reason) in the order they closed, as ``SegmentResult.spans``."""
    out = []
    entries = ring(state)
    capacity = entries.shape[1]
    for b, rec in enumerate(np.asarray(state)):
        frames, open_start, count = int(rec[0]), int(rec[3]), int(rec[4])
        row = [tuple(int(v) for v in entries[b, k % capacity, :3]) for k in range(count - min(count, capacity), count)]
        if include_open and open_start >= 0:
            row.append((open_start, frames, -1))
        out.append(row)
    return out
