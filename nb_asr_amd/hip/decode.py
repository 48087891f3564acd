"""The steps after the logits: CTC post-processing and greedy streaming, the beam search (whole, streaming, peeked; plain, timed, fused),
token error counts, the CTC loss with its gradient, forced alignment."""
import ctypes
import operator

import torch

from . import (SIGNATURES, HipError, load_library, _call, _scratch, _opaque, _stream, _dev, _ptr, _state, _int_tensor, _lengths_ptr,
               _c_float_p, _c_int, _c_stream)

SIGNATURES.update({
    'nbasr_ctc_postprocess': (_c_int, [_c_float_p] * 5 + [_c_int] * 4 + [_c_stream]),
    'nbasr_ctc_greedy_stream': (_c_int, [_c_float_p] * 4 + [_c_int] * 4 + [_c_stream]),
    'nbasr_ctc_loss': (_c_int, [_c_float_p] * 5 + [_c_int] * 6 + [_c_stream]),
    'nbasr_ctc_grad_workspace_bytes': (ctypes.c_size_t, [_c_int] * 3),
    'nbasr_ctc_loss_grad': (_c_int, [_c_float_p] * 7 + [_c_int] * 5 + [_c_stream]),
    'nbasr_ctc_align_workspace_bytes': (ctypes.c_size_t, [_c_int] * 3),
    'nbasr_ctc_forced_align': (_c_int, [_c_float_p] * 10 + [_c_int] * 5 + [_c_stream]),
    'nbasr_ctc_beam_workspace_bytes': (ctypes.c_size_t, [_c_int] * 4),
    'nbasr_ctc_beam_search': (_c_int, [_c_float_p] * 6 + [_c_int] * 6 + [_c_stream]),
    'nbasr_token_error_counts': (_c_int, [_c_float_p, _c_float_p, _c_int, _c_float_p, _c_float_p, _c_int, _c_float_p, _c_int, _c_int,
                                          _c_float_p, _c_int, _c_stream]),
    'nbasr_ctc_beam_stream_state_bytes': (ctypes.c_size_t, [_c_int] * 3),
    'nbasr_ctc_beam_stream_workspace_bytes': (ctypes.c_size_t, [_c_int] * 4),
    'nbasr_ctc_beam_stream_init': (_c_int, [ctypes.c_void_p] + [_c_int] * 3 + [_c_stream]),
    'nbasr_ctc_beam_stream_step': (_c_int, [_c_float_p] * 9 + [_c_int] * 7 + [_c_stream]),
    'nbasr_ctc_beam_stream_finish': (_c_int, [ctypes.c_void_p] + [_c_float_p] * 3 + [_c_int] * 4 + [_c_stream]),
    'nbasr_ctc_beam_timed_workspace_bytes': (ctypes.c_size_t, [_c_int] * 4),
    'nbasr_ctc_beam_search_timed': (_c_int, [_c_float_p] * 7 + [_c_int] * 6 + [_c_stream]),
    'nbasr_ctc_beam_stream_timed_state_bytes': (ctypes.c_size_t, [_c_int] * 3),
    'nbasr_ctc_beam_stream_timed_init': (_c_int, [ctypes.c_void_p] + [_c_int] * 3 + [_c_stream]),
    'nbasr_ctc_beam_stream_timed_step': (_c_int, [_c_float_p] * 11 + [_c_int] * 7 + [_c_stream]),
    'nbasr_ctc_beam_stream_timed_finish': (_c_int, [ctypes.c_void_p] + [_c_float_p] * 4 + [_c_int] * 4 + [_c_stream]),
    'nbasr_ctc_beam_stream_peek_workspace_bytes': (ctypes.c_size_t, [_c_int] * 5),
    'nbasr_ctc_beam_stream_peek': (_c_int, [_c_float_p] * 2 + [ctypes.c_void_p] + [_c_float_p] * 4 + [_c_int] * 8 + [_c_stream]),
    'nbasr_ctc_beam_stream_timed_peek': (_c_int, [_c_float_p] * 2 + [ctypes.c_void_p] + [_c_float_p] * 5 + [_c_int] * 8 + [_c_stream]),
    'nbasr_ctc_beam_search_lm': (_c_int, [_c_float_p] * 8 + [_c_int] * 7 + [_c_stream]),
    'nbasr_ctc_beam_stream_lm_step': (_c_int, [_c_float_p] * 12 + [_c_int] * 8 + [_c_stream]),
    'nbasr_ctc_beam_stream_lm_peek': (_c_int, [_c_float_p] * 3 + [ctypes.c_void_p] + [_c_float_p] * 5 + [_c_int] * 9 + [_c_stream]),
})


def ctc_postprocess(logits, lengths=None, want_log_probs=True, want_tokens=True, blank=0):
    """logits (B, T', C) -> (log_probs or None, tokens (B, T') int32 padded with -1 or None, token_counts (B) or None)."""
    _dev(logits, 'logits')
    b, t, c = logits.shape
    log_probs = torch.empty_like(logits) if want_log_probs else None
    tokens = torch.empty(b, t, dtype=torch.int32, device=logits.device) if want_tokens else None
    counts = torch.empty(b, dtype=torch.int32, device=logits.device) if want_tokens else None
    _call('nbasr_ctc_postprocess', logits.data_ptr(), _lengths_ptr(lengths, b), _ptr(log_probs), _ptr(tokens), _ptr(counts), b, t, c, blank, _stream(logits))
    return log_probs, tokens, counts


def ctc_greedy_stream(logits, prev, blank=0):
    """Greedy CTC decoding of one chunk of a stream: logits (B, n, C) float32; ``prev`` (B) int32 device tensor, in/out: the argmax of
    the frame before the chunk (-1 at an utterance's start), replaced by the chunk's last one.  Returns (tokens (B, n) int32 padded
    with -1, token_counts (B) int32); repeats are collapsed across chunk boundaries (nbasr.h: nbasr_ctc_greedy_stream)."""
    _dev(logits, 'logits')
    b, t, c = logits.shape
    _int_tensor(prev, 'prev', logits.device, (b,))
    tokens = torch.empty(b, t, dtype=torch.int32, device=logits.device)
    counts = torch.empty(b, dtype=torch.int32, device=logits.device)
    _call('nbasr_ctc_greedy_stream', logits.data_ptr() if t else None, prev.data_ptr(), tokens.data_ptr() if t else None, counts.data_ptr(),
          b, t, c, blank, _stream(logits))
    return tokens, counts


# The beam entry points.  Per operation: the name of its entry points -- {} = '' plain, '_timed', '_lm' fused (only where the list has
# ``fusion``) -- and its widest argument list, in the order of include/nbasr.h.  The fused entry point takes the whole list; the timed
# one all but ``fusion`` and ``timed``; the plain one drops the timed-only outputs as well.
_BEAM_OPS = {
    'search': ('nbasr_ctc_beam_search{}',
               'log_probs lengths fusion ws beams scores timesteps beam_lens batch frames classes beam_width blank cutoff_top_n timed stream'),
    'step': ('nbasr_ctc_beam_stream{}_step', 'log_probs chunk_lengths fusion state ws committed committed_frames committed_counts partial '
             'partial_frames partial_counts usage batch frames classes beam_width blank cutoff_top_n pool_nodes timed stream'),
    'peek': ('nbasr_ctc_beam_stream{}_peek', 'log_probs chunk_lengths fusion state ws beams scores timesteps beam_lens ld_beams batch frames '
             'classes beam_width blank cutoff_top_n pool_nodes timed stream'),
    'finish': ('nbasr_ctc_beam_stream{}_finish', 'state beams scores timesteps beam_lens ld_beams batch beam_width pool_nodes stream'),
    'init': ('nbasr_ctc_beam_stream{}_init', 'state batch beam_width pool_nodes stream'),
}
# (operation, timed, fused) -> (entry point, the names of its arguments in order): every beam call the binding can make
BEAM_ENTRY_POINTS = {}
for _op, (_name, _args) in _BEAM_OPS.items():
    _unfused = [n for n in _args.split() if n not in ('fusion', 'timed')]
    BEAM_ENTRY_POINTS[_op, False, False] = (_name.format(''), [n for n in _unfused if n not in ('timesteps', 'committed_frames', 'partial_frames')])
    BEAM_ENTRY_POINTS[_op, True, False] = (_name.format('_timed'), _unfused)
    if 'fusion' in _args.split():
        BEAM_ENTRY_POINTS[_op, False, True] = BEAM_ENTRY_POINTS[_op, True, True] = (_name.format('_lm'), _args.split())
_BEAM_PICKERS = {key: (name, operator.itemgetter(*names)) for key, (name, names) in BEAM_ENTRY_POINTS.items()}


def _beam_call(op, timesteps, fused, values):
    """One call of the entry point of ``BEAM_ENTRY_POINTS`` for (op, timesteps, fused), its arguments picked from ``values`` by name (a
    fused, untimed call passes NULL for the timed-only outputs)."""
    name, pick = _BEAM_PICKERS[op, bool(timesteps), fused]
    _call(name, *pick(values))


def _fusion(fusion, classes, device):
    """A fusion table as the fused entry points read it: contiguous float32 (classes, classes) on the device of the log-probabilities
    (``ctc.fusion_table`` makes and validates one)."""
    if (not isinstance(fusion, torch.Tensor) or fusion.dtype != torch.float32 or fusion.device != device or not fusion.is_contiguous()
            or tuple(fusion.shape) != (classes, classes)):
        raise HipError(f'fusion must be a contiguous float32 tensor ({classes}, {classes}) on {device} (ctc.fusion_table)')
    return fusion


def _check_chunk(log_probs, lengths, fusion, lengths_name='lengths'):
    """The one check of a chunk of log-probabilities (B, n, C) float32 with its int32 lengths (B) or None and its fusion table or None.
    -> (B, n, C, the device)"""
    _dev(log_probs, 'log_probs')
    b, t, c = log_probs.shape
    if fusion is not None:
        _fusion(fusion, c, log_probs.device)
    if lengths is not None:
        _int_tensor(lengths, lengths_name, log_probs.device, (b,))
    return b, t, c, log_probs.device


def _check_stream_chunk(who, log_probs, chunk_lengths, fusion, state, beam_width, pool_nodes, timesteps):
    """``_check_chunk`` for the streaming wrapper ``who``, and that ``state`` is one of its family's size on the same device."""
    b, t, c, dev = _check_chunk(log_probs, chunk_lengths, fusion, 'chunk_lengths')
    _state(state)                      # (its words for a tensor off the device or not contiguous; the size below)
    _opaque(state, ctc_beam_stream_state_bytes(b, beam_width, pool_nodes, timesteps),
            ('{}: state must be a tensor of ctc_beam_stream_state_bytes bytes on the device of log_probs', who), dtype=None, device=dev)
    return b, t, c, dev


def _beam_outputs(batch, beam_width, ld, timesteps, device):
    """The outputs of a search, a finish or a peek, allocated: (beams (B, W, ld), scores, timesteps like beams | None, beam_lens)."""
    beams = torch.empty(batch, beam_width, ld, dtype=torch.int32, device=device)
    scores = torch.empty(batch, beam_width, dtype=torch.float32, device=device)
    lens = torch.empty(batch, beam_width, dtype=torch.int32, device=device)
    steps = torch.empty_like(beams) if timesteps else None
    return beams, scores, steps, lens


def beam_result(beams, scores, timesteps, beam_lens):
    """The four slots of a beam result as the public tuple: ``(beams, scores, timesteps, beam_lens)``, without time steps (None)
    ``(beams, scores, beam_lens)``."""
    return (beams, scores, beam_lens) if timesteps is None else (beams, scores, timesteps, beam_lens)


def ctc_beam_search(log_probs, lengths=None, beam_width=12, blank=0, cutoff_top_n=40, timesteps=False, fusion=None):
    """log_probs (B, T', C) float32 log-probabilities -> (beams (B, W, T') int32 best first, scores (B, W) = -log P,
    beam_lens (B, W) int32).  ``lengths``: int32 device tensor (B) of valid output frames, or None.  ``timesteps``: the timed search
    (nbasr_ctc_beam_search_timed) -> (beams, scores, timesteps (B, W, T') int32, beam_lens).  ``fusion``: a fusion table (C, C) float32 on
    the device (nbasr.h "bigram LM fusion"): the fused search, nbasr_ctc_beam_search_lm, timed or not; None: the entry points above."""
    b, t, c, dev = _check_chunk(log_probs, lengths, fusion)
    beams, scores, steps, lens = outs = _beam_outputs(b, beam_width, t, timesteps, dev)
    lib = load_library()
    ws_bytes = lib.nbasr_ctc_beam_timed_workspace_bytes if timesteps else lib.nbasr_ctc_beam_workspace_bytes
    ws = _scratch(ws_bytes(b, t, c, beam_width), dev, torch.int64)              # (B * T' * C floats may be an odd count of words)
    _beam_call('search', timesteps, fusion is not None, {
        'log_probs': log_probs.data_ptr(), 'lengths': _ptr(lengths), 'fusion': _ptr(fusion), 'ws': ws.data_ptr(), 'beams': beams.data_ptr(),
        'scores': scores.data_ptr(), 'timesteps': _ptr(steps), 'beam_lens': lens.data_ptr(), 'batch': b, 'frames': t, 'classes': c,
        'beam_width': beam_width, 'blank': blank, 'cutoff_top_n': cutoff_top_n, 'timed': 1 if timesteps else 0, 'stream': _stream(log_probs)})
    return beam_result(*outs)


def ctc_beam_stream_state_bytes(batch, beam_width, pool_nodes, timesteps=False):
    """Bytes of the state of a streaming beam search (nbasr.h: nbasr_ctc_beam_stream_state_bytes, or _timed_state_bytes); 0 for bad sizes."""
    lib = load_library()
    fn = lib.nbasr_ctc_beam_stream_timed_state_bytes if timesteps else lib.nbasr_ctc_beam_stream_state_bytes
    return int(fn(batch, beam_width, pool_nodes))


def ctc_beam_stream_init(state, batch, beam_width, pool_nodes, timesteps=False):
    """Every utterance of ``state`` (a device tensor of ``ctc_beam_stream_state_bytes`` bytes) to the empty prefix."""
    ptr = _state(state)
    _opaque(state, ctc_beam_stream_state_bytes(batch, beam_width, pool_nodes, timesteps),
            'ctc_beam_stream_init: state tensor too small (ctc_beam_stream_state_bytes)', dtype=None)
    _beam_call('init', timesteps, False, {'state': ptr, 'batch': batch, 'beam_width': beam_width, 'pool_nodes': pool_nodes, 'stream': _stream(state)})


def ctc_beam_stream_step(log_probs, chunk_lengths, state, beam_width, pool_nodes, blank=0, cutoff_top_n=40, timesteps=False, fusion=None):
    """One chunk of a streaming beam search (nbasr.h: nbasr_ctc_beam_stream_step): log_probs (B, n, C) float32, chunk_lengths (B) int32 device tensor or None.
    Returns device tensors (committed (B, pool_nodes), partial (B, pool_nodes), counts (3, B) int32 = committed counts, partial counts, pool usage (-1:
    refused, the pool is too small for this chunk)).  ``timesteps`` (a state of the timed family, nbasr_ctc_beam_stream_timed_step): (committed, partial,
    committed_frames, partial_frames, counts).  ``fusion``: as ``ctc_beam_search`` takes it (nbasr_ctc_beam_stream_lm_step, over a state of either family)."""
    b, t, c, dev = _check_stream_chunk('ctc_beam_stream_step', log_probs, chunk_lengths, fusion, state, beam_width, pool_nodes, timesteps)
    rows = torch.empty(4 if timesteps else 2, b, pool_nodes, dtype=torch.int32, device=dev).unbind(0)
    counts = torch.empty(3, b, dtype=torch.int32, device=dev)
    ws = _scratch(load_library().nbasr_ctc_beam_stream_workspace_bytes(b, t, c, pool_nodes), dev, torch.int32)
    count_ptr = counts.data_ptr()                              # its rows: committed counts, partial counts, usage, 4 * b bytes each
    _beam_call('step', timesteps, fusion is not None, {
        'log_probs': log_probs.data_ptr() if t else None, 'chunk_lengths': _ptr(chunk_lengths), 'fusion': _ptr(fusion), 'state': _state(state),
        'ws': ws.data_ptr(), 'committed': rows[0].data_ptr(), 'committed_frames': rows[2].data_ptr() if timesteps else None,
        'committed_counts': count_ptr, 'partial': rows[1].data_ptr(), 'partial_frames': rows[3].data_ptr() if timesteps else None,
        'partial_counts': count_ptr + 4 * b, 'usage': count_ptr + 8 * b, 'batch': b, 'frames': t, 'classes': c, 'beam_width': beam_width,
        'blank': blank, 'cutoff_top_n': cutoff_top_n, 'pool_nodes': pool_nodes, 'timed': 1 if timesteps else 0, 'stream': _stream(log_probs)})
    return (*rows, counts)


def ctc_beam_stream_finish(state, batch, beam_width, pool_nodes, ld, timesteps=False):
    """The live prefixes' uncommitted suffixes (nbasr.h: nbasr_ctc_beam_stream_finish): (suffixes (B, W, ld) int32, scores (B, W),
    suffix lengths (B, W) int32, -1 beyond the live prefixes).  ``timesteps`` (nbasr_ctc_beam_stream_timed_finish): (suffixes, scores,
    the suffix tokens' frames (B, W, ld) int32, suffix lengths)."""
    beams, scores, steps, lens = outs = _beam_outputs(batch, beam_width, max(int(ld), 1), timesteps, state.device)
    _beam_call('finish', timesteps, False, {
        'state': _state(state), 'beams': beams.data_ptr(), 'scores': scores.data_ptr(), 'timesteps': _ptr(steps), 'beam_lens': lens.data_ptr(),
        'ld_beams': beams.shape[2], 'batch': batch, 'beam_width': beam_width, 'pool_nodes': pool_nodes, 'stream': _stream(state)})
    return beam_result(*outs)


def ctc_beam_stream_peek_workspace_bytes(batch, frames, classes, beam_width, pool_nodes):
    """Bytes of the workspace of ``ctc_beam_stream_peek`` (nbasr.h: nbasr_ctc_beam_stream_peek_workspace_bytes, one size for both families);
    0 for sizes beyond the limits."""
    return int(load_library().nbasr_ctc_beam_stream_peek_workspace_bytes(int(batch), int(frames), int(classes), int(beam_width), int(pool_nodes)))


def ctc_beam_stream_peek(log_probs, chunk_lengths, state, beam_width, pool_nodes, ld, blank=0, cutoff_top_n=40, timesteps=False, ws=None,
                         fusion=None):
    """What ``ctc_beam_stream_finish`` would return after a ``ctc_beam_stream_step`` of this chunk, with ``state`` only read (nbasr.h:
    nbasr_ctc_beam_stream_peek, ``timesteps``: nbasr_ctc_beam_stream_timed_peek): log_probs (B, n, C) float32, n >= 0; returns
    ``ctc_beam_stream_finish``'s tuple with suffixes (B, W, ld).  ``ws``: a device tensor of ``ctc_beam_stream_peek_workspace_bytes`` bytes
    to use (None: one is allocated).  ``fusion``: as ``ctc_beam_search`` takes it (nbasr_ctc_beam_stream_lm_peek)."""
    b, t, c, dev = _check_stream_chunk('ctc_beam_stream_peek', log_probs, chunk_lengths, fusion, state, beam_width, pool_nodes, timesteps)
    need = ctc_beam_stream_peek_workspace_bytes(b, t, c, beam_width, pool_nodes)
    if ws is None:
        ws = _scratch(need, dev, torch.int64)
    else:
        _opaque(ws, need, ('ctc_beam_stream_peek: the workspace must be a contiguous tensor of {} bytes on {}', need, dev), dtype=None, device=dev)
    beams, scores, steps, lens = outs = _beam_outputs(b, beam_width, max(int(ld), 1), timesteps, dev)
    _beam_call('peek', timesteps, fusion is not None, {
        'log_probs': log_probs.data_ptr() if t else None, 'chunk_lengths': _ptr(chunk_lengths), 'fusion': _ptr(fusion), 'state': _state(state),
        'ws': ws.data_ptr(), 'beams': beams.data_ptr(), 'scores': scores.data_ptr(), 'timesteps': _ptr(steps), 'beam_lens': lens.data_ptr(),
        'ld_beams': beams.shape[2], 'batch': b, 'frames': t, 'classes': c, 'beam_width': beam_width, 'blank': blank,
        'cutoff_top_n': cutoff_top_n, 'pool_nodes': pool_nodes, 'timed': 1 if timesteps else 0, 'stream': _stream(log_probs)})
    return beam_result(*outs)


def token_error_counts(hyp, hyp_len, ref, ref_len, table=None, blank=0):
    """hyp (B, Lh), ref (B, Lr) int32 label matrices with their lengths (B) -> counts (B, 2) int32 = (Levenshtein distance,
    reference length) after mapping through ``table`` (int32, optional) and dropping ``blank``."""
    if hyp.dim() != 2 or ref.dim() != 2 or hyp.shape[0] != ref.shape[0]:
        raise HipError('hyp and ref must be (batch, length) matrices over the same batch')
    dev = hyp.device
    b = hyp.shape[0]
    for t, what in ((hyp, 'hyp'), (ref, 'ref')):
        _int_tensor(t, what, dev)
    _int_tensor(hyp_len, 'hyp_len', dev, (b,))
    _int_tensor(ref_len, 'ref_len', dev, (b,))
    if table is not None:
        _int_tensor(table, 'table', dev)
    counts = torch.empty(b, 2, dtype=torch.int32, device=dev)
    _call('nbasr_token_error_counts', hyp.data_ptr(), hyp_len.data_ptr(), hyp.shape[1], ref.data_ptr(), ref_len.data_ptr(), ref.shape[1],
          _ptr(table), 0 if table is None else table.numel(), blank, counts.data_ptr(), b, torch.cuda.current_stream(dev).cuda_stream)
    return counts


def _ctc_args(log_probs, lengths, targets, target_lengths):
    _dev(log_probs, 'log_probs')
    b, t, c = log_probs.shape
    dev = log_probs.device
    _int_tensor(lengths, 'lengths', dev, (b,))
    _int_tensor(target_lengths, 'target_lengths', dev, (b,))
    _int_tensor(targets, 'targets', dev)
    if targets.dim() != 2 or targets.shape[0] != b:
        raise HipError(f'targets must be (batch, labels), got {tuple(targets.shape)}')
    return b, t, c, dev


def ctc_loss(log_probs, lengths, targets, target_lengths, blank=0, divide_by_length=False):
    """log_probs (B, T', C) float32, lengths (B) int32, targets (B, L) int32, target_lengths (B) int32 (all on the device)
    -> per-utterance negative log-likelihood (B) float32 with zero_infinity semantics, optionally divided by ``lengths``."""
    b, t, c, dev = _ctc_args(log_probs, lengths, targets, target_lengths)
    losses = torch.empty(b, dtype=torch.float32, device=dev)
    _call('nbasr_ctc_loss', log_probs.data_ptr(), lengths.data_ptr(), targets.data_ptr(), target_lengths.data_ptr(), losses.data_ptr(), b, t, c,
          targets.shape[1], blank, 1 if divide_by_length else 0, _stream(log_probs))
    return losses


def ctc_loss_grad(log_probs, lengths, targets, target_lengths, blank=0):
    """-> (per-utterance loss / length (B), d mean(loss / length) / d logits (B, T', C)) for log_probs = log_softmax(logits)."""
    b, t, c, dev = _ctc_args(log_probs, lengths, targets, target_lengths)
    losses = torch.empty(b, dtype=torch.float32, device=dev)
    grad = torch.empty_like(log_probs)
    ws = _scratch(load_library().nbasr_ctc_grad_workspace_bytes(b, t, targets.shape[1]), dev)
    _call('nbasr_ctc_loss_grad', log_probs.data_ptr(), lengths.data_ptr(), targets.data_ptr(), target_lengths.data_ptr(), ws.data_ptr(),
          losses.data_ptr(), grad.data_ptr(), b, t, c, targets.shape[1], blank, _stream(log_probs))
    return losses, grad


def ctc_forced_align(log_probs, lengths, targets, target_lengths, blank=0):
    """The best CTC path of each transcript (nbasr.h: nbasr_ctc_forced_align; arguments as ``ctc_loss``) -> (scores (B) float32,
    path (B, T') int32, starts (B, L) int32, ends (B, L) int32, token_scores (B, L) float32)."""
    b, t, c, dev = _ctc_args(log_probs, lengths, targets, target_lengths)
    ld = targets.shape[1]
    scores = torch.empty(b, dtype=torch.float32, device=dev)
    path = torch.empty(b, t, dtype=torch.int32, device=dev)
    starts, ends = torch.empty(b, ld, dtype=torch.int32, device=dev), torch.empty(b, ld, dtype=torch.int32, device=dev)
    token_scores = torch.empty(b, ld, dtype=torch.float32, device=dev)
    ws = _scratch(load_library().nbasr_ctc_align_workspace_bytes(b, t, ld), dev)
    _call('nbasr_ctc_forced_align', log_probs.data_ptr(), lengths.data_ptr(), targets.data_ptr(), target_lengths.data_ptr(), ws.data_ptr(),
          scores.data_ptr(), path.data_ptr(), starts.data_ptr(), ends.data_ptr(), token_scores.data_ptr(), b, t, c, ld, blank, _stream(log_probs))
    return scores, path, starts, ends, token_scores
