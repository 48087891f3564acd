"""The detectors over CTC logits: the endpoint, segment, keyword and confidence steps and the sizes of their states."""
import ctypes

import torch

from . import SIGNATURES, HipError, load_library, _call, _stream, _dev, _ptr, _int_tensor, _c_float_p, _c_int, _c_stream

SIGNATURES.update({
    'nbasr_ctc_endpoint_state_bytes': (ctypes.c_size_t, [_c_int]),
    'nbasr_ctc_endpoint_step': (_c_int, [_c_float_p] * 5 + [_c_int, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_float, ctypes.c_void_p]
                                + [_c_int] * 3 + [_c_stream]),
    'nbasr_ctc_segment_state_bytes': (ctypes.c_size_t, [_c_int, _c_int]),
    'nbasr_ctc_segment_step': (_c_int, [_c_float_p] * 4 + [_c_int] * 4 + [ctypes.c_longlong, ctypes.c_longlong, ctypes.c_float, ctypes.c_void_p]
                               + [_c_int] * 3 + [_c_stream]),
    'nbasr_ctc_keyword_state_bytes': (ctypes.c_size_t, [_c_int, _c_int]),
    'nbasr_ctc_keyword_step': (_c_int, [_c_float_p] * 5 + [_c_int] * 2 + [_c_float_p] * 4 + [_c_int] * 3 + [_c_stream]),
    'nbasr_ctc_confidence_state_bytes': (ctypes.c_size_t, [_c_int]),
    'nbasr_ctc_confidence_step': (_c_int, [_c_float_p] * 5 + [_c_int, ctypes.c_float, _c_int, _c_int] + [_c_float_p] * 3 + [_c_int] * 3 + [_c_stream]),
})

ENDPOINT_STATE_WORDS = 8         # int32 per utterance: frames, speech_frames, first_speech, last_speech, endpoint_frame, endpoint_rule, 0, 0


def ctc_endpoint_state_bytes(batch):
    """Bytes of the endpoint state of ``batch`` utterances (nbasr.h: nbasr_ctc_endpoint_state_bytes); 0 for a batch that is not positive."""
    return int(load_library().nbasr_ctc_endpoint_state_bytes(int(batch)))


def _signed64(word):
    """An unsigned 64-bit pattern as the ``long long`` that carries it by value."""
    word = int(word) & 0xFFFFFFFFFFFFFFFF
    return word - (1 << 64) if word >> 63 else word


def _detector_step_args(who, x, lengths, state_in, state_out, words, k=None):
    """The checks the detector steps share: ``x`` (B, n, C) float32 on the device, ``state_out`` and (unless None) ``state_in``
    contiguous int32 (B, words) or (B, k, words), ``lengths`` None or int32 (B).  -> (B, n, C)."""
    _dev(x, 'x')
    shape, dev = x.shape, x.device               # (read once: a step is host-bound)
    if len(shape) != 3:
        raise HipError(f'{who}: x must be (batch, frames, classes), got {tuple(shape)}')
    b = shape[0]
    record = (b, words) if k is None else (b, k, words)
    _int_tensor(state_out, 'state_out', dev, record)
    if state_in is not None:
        _int_tensor(state_in, 'state_in', dev, record)
    if lengths is not None:
        _int_tensor(lengths, 'lengths', dev, (b,))
    return shape


def ctc_endpoint_step(x, lengths, state_in, state_out, rules, speech_lo, speech_hi, margin, mask_out=None):
    """One step of the endpointer (nbasr.h: nbasr_ctc_endpoint_step) over ``x`` (B, n, C) float32 logits or log-probabilities.  ``lengths``: int32 device
    tensor (B) or None.  ``state_in`` / ``state_out``: (B, 8) int32 device tensors -- ``state_in`` None starts fresh rows, the same tensor twice commits in
    place, two tensors leave ``state_in`` as it was.  ``rules``: (n_rules, 3) int32 device table; ``speech_lo`` / ``speech_hi``: the class mask's two 64-bit
    words; ``mask_out``: (B, n) uint8 device tensor or None.  Returns ``state_out``."""
    b, n, c = _detector_step_args('ctc_endpoint_step', x, lengths, state_in, state_out, ENDPOINT_STATE_WORDS)
    _int_tensor(rules, 'rules', x.device, (rules.shape[0], 3))
    _call('nbasr_ctc_endpoint_step', x.data_ptr() if x.numel() else None, _ptr(lengths), _ptr(state_in), state_out.data_ptr(), rules.data_ptr(), rules.shape[0],
          _signed64(speech_lo), _signed64(speech_hi), float(margin), _speech_mask_arg('ctc_endpoint_step', mask_out, x), b, n, c, _stream(x))
    return state_out


def _speech_mask_arg(who, mask_out, x):
    """The address of a step's ``mask_out`` -- None, or a contiguous (B, n) uint8 tensor beside ``x`` (B, n, C) -- or None."""
    if mask_out is None:
        return None
    b, n = x.shape[:2]
    if mask_out.dtype != torch.uint8 or mask_out.device != x.device or tuple(mask_out.shape) != (b, n) or not mask_out.is_contiguous():
        raise HipError(f'{who}: mask_out must be a contiguous ({b}, {n}) uint8 tensor on {x.device}')
    return mask_out.data_ptr() if mask_out.numel() else None


SEGMENT_HEAD_WORDS = 8           # int32 per utterance ahead of the ring: frames, speech_run, silence_run, open_start, count, 0, 0, 0
SEGMENT_ENTRY_WORDS = 4          # a ring entry: start, end, reason, 0
SEGMENT_MAX_CAPACITY = 64


def ctc_segment_state_words(capacity):
    """int32 words of one utterance's segment record with a ring of ``capacity`` entries: 8 + 4 capacity."""
    return SEGMENT_HEAD_WORDS + SEGMENT_ENTRY_WORDS * int(capacity)


def ctc_segment_state_bytes(batch, capacity):
    """Bytes of the segment state of ``batch`` utterances with rings of ``capacity`` entries (nbasr.h: nbasr_ctc_segment_state_bytes);
    0 for a batch that is not positive or a capacity outside [1, 64]."""
    return int(load_library().nbasr_ctc_segment_state_bytes(int(batch), int(capacity)))


def ctc_segment_step(x, lengths, state_in, state_out, min_speech, min_silence, max_frames, capacity, speech_lo, speech_hi, margin, mask_out=None):
    """One step of the segmenter (nbasr.h: nbasr_ctc_segment_step) over ``x`` (B, n, C) float32 logits or log-probabilities.  ``lengths``: int32 device tensor
    (B) or None.  ``state_in`` / ``state_out``: (B, 8 + 4 capacity) int32 device tensors -- ``state_in`` None starts fresh rows, the same tensor twice commits
    in place, two tensors leave ``state_in`` as it was.  ``min_speech``, ``min_silence``, ``max_frames``, ``capacity``: the counts, by value; ``speech_lo`` /
    ``speech_hi``: the class mask's two 64-bit words; ``mask_out``: (B, n) uint8 device tensor or None.  Returns ``state_out``."""
    capacity = int(capacity)
    if not 1 <= capacity <= SEGMENT_MAX_CAPACITY:
        raise HipError(f'ctc_segment_step: capacity={capacity} must lie in [1, {SEGMENT_MAX_CAPACITY}]')
    b, n, c = _detector_step_args('ctc_segment_step', x, lengths, state_in, state_out, ctc_segment_state_words(capacity))
    _call('nbasr_ctc_segment_step', x.data_ptr() if x.numel() else None, _ptr(lengths), _ptr(state_in), state_out.data_ptr(), int(min_speech),
          int(min_silence), int(max_frames), capacity, _signed64(speech_lo), _signed64(speech_hi), float(margin),
          _speech_mask_arg('ctc_segment_step', mask_out, x), b, n, c, _stream(x))
    return state_out


KEYWORD_STATE_WORDS = 136        # 32-bit words per (utterance, keyword): frames, hit (frame, start, score), best (frame, start, score), 0, V[64], start[64]
KEYWORD_MAX_TOKENS = 32          # the pitch of the token table


def ctc_keyword_state_bytes(batch, n_keywords):
    """Bytes of the keyword state of ``batch`` utterances and ``n_keywords`` keywords (nbasr.h: nbasr_ctc_keyword_state_bytes); 0 when
    either is not positive."""
    return int(load_library().nbasr_ctc_keyword_state_bytes(int(batch), int(n_keywords)))


def ctc_keyword_step(x, lengths, tokens, token_counts, thresholds, blank, state_in, state_out, scores_out=None, starts_out=None):
    """One step of the keyword spotter (nbasr.h: nbasr_ctc_keyword_step) over ``x`` (B, n, C) float32 logits or log-probabilities.  ``lengths``: int32 device
    tensor (B) or None.  ``tokens``: (K, 32) int32 device table, -1 past a keyword's end; ``token_counts``:  (K) int32; ``thresholds``: (K) float32.
    ``state_in`` / ``state_out``: (B, K, 136) int32 device tensors -- ``state_in`` None starts fresh rows, the same tensor twice commits in place, two tensors
    leave ``state_in`` as it was.  ``scores_out`` / ``starts_out``:  (B, K, n) float32 / int32 device tensors, both or neither.  Returns ``state_out``."""
    k = tokens.shape[0]
    b, n, c = _detector_step_args('ctc_keyword_step', x, lengths, state_in, state_out, KEYWORD_STATE_WORDS, k)
    _int_tensor(tokens, 'tokens', x.device, (k, KEYWORD_MAX_TOKENS))
    _int_tensor(token_counts, 'token_counts', x.device, (k,))
    _dev(thresholds, 'thresholds')
    if thresholds.device != x.device or tuple(thresholds.shape) != (k,):
        raise HipError(f'ctc_keyword_step: thresholds must have shape ({k},) on {x.device}')
    if (scores_out is None) != (starts_out is None):
        raise HipError('ctc_keyword_step: the trace is scores_out and starts_out together: give both or neither')
    if scores_out is not None:
        _dev(scores_out, 'scores_out')
        if scores_out.device != x.device or tuple(scores_out.shape) != (b, k, n):
            raise HipError(f'ctc_keyword_step: scores_out must have shape ({b}, {k}, {n}) on {x.device}')
        _int_tensor(starts_out, 'starts_out', x.device, (b, k, n))
    trace = scores_out is not None and scores_out.numel() > 0
    _call('nbasr_ctc_keyword_step', x.data_ptr() if x.numel() else None, _ptr(lengths), tokens.data_ptr(), token_counts.data_ptr(),
          thresholds.data_ptr(), k, int(blank), _ptr(state_in), state_out.data_ptr(), scores_out.data_ptr() if trace else None,
          starts_out.data_ptr() if trace else None, b, n, c, _stream(x))
    return state_out


CONFIDENCE_STATE_WORDS = 16      # int32 per utterance: frames, prev_label, open_start, open_min_q, open_sum (lo, hi), tokens, utt_min_q, utt_sum (lo, hi), utt_frames, bad, 0 x 4
CONFIDENCE_TOKEN_WORDS = 8       # a closed token: label, start, end, min_q, sum_lo, sum_hi, 0, 0
CONFIDENCE_MEASURES = ('prob', 'entropy', 'tsallis')         # ``measure`` by value: the index


def ctc_confidence_state_bytes(batch):
    """Bytes of the confidence state of ``batch`` utterances (nbasr.h: nbasr_ctc_confidence_state_bytes); 0 for a batch that is not positive."""
    return int(load_library().nbasr_ctc_confidence_state_bytes(int(batch)))


def ctc_confidence_step(x, lengths, path, state_in, state_out, measure, alpha, blank, final, tokens_out=None, token_counts=None, frame_q=None):
    """One step of the confidence estimator (nbasr.h: nbasr_ctc_confidence_step) over ``x`` (B, n, C) float32 logits or log-probabilities.  ``lengths``: int32
    device tensor (B) or None; ``path``: (B, n) int32 device tensor, the labels of a hypothesis, or None (the greedy labels).  ``state_in`` / ``state_out``:
    (B, 16) int32 device tensors -- ``state_in`` None starts fresh rows, the same tensor twice commits in place, two tensors leave ``state_in`` as it was.
    ``measure`` (0 prob, 1 entropy, 2 tsallis), ``alpha``, ``blank``, ``final``: by value.  ``tokens_out`` (B, n + 1, 8) and ``token_counts`` (B) int32, both or
    neither: the tokens this step closed; ``frame_q``: (B, n) int32 or None, every frame's quantised confidence.  Returns ``state_out``."""
    b, n, c = _detector_step_args('ctc_confidence_step', x, lengths, state_in, state_out, CONFIDENCE_STATE_WORDS)
    if path is not None:
        _int_tensor(path, 'path', x.device, (b, n))
    if (tokens_out is None) != (token_counts is None):
        raise HipError('ctc_confidence_step: the tokens are tokens_out and token_counts together: give both or neither')
    if tokens_out is not None:
        _int_tensor(tokens_out, 'tokens_out', x.device, (b, n + 1, CONFIDENCE_TOKEN_WORDS))
        _int_tensor(token_counts, 'token_counts', x.device, (b,))
    if frame_q is not None:
        _int_tensor(frame_q, 'frame_q', x.device, (b, n))
    some = x.numel() > 0
    _call('nbasr_ctc_confidence_step', x.data_ptr() if some else None, _ptr(lengths), path.data_ptr() if path is not None and some else None,
          _ptr(state_in), state_out.data_ptr(), int(measure), float(alpha), int(blank), int(bool(final)), _ptr(tokens_out), _ptr(token_counts),
          frame_q.data_ptr() if frame_q is not None and some else None, b, n, c, _stream(x))
    return state_out
