"""The front-end's entry points: framing, the DFT / filterbank GEMM, power, log-normalisation, the front-end stream, the resampler."""
import ctypes

import torch

from . import SIGNATURES, HipError, load_library, _call, _stream, _dev, _opt, _lengths_ptr, round_up4, _c_float_p, _c_int, _c_stream

SIGNATURES.update({
    'nbasr_pointwise_linear': (_c_int, [_c_float_p] * 4 + [_c_int] * 6 + [_c_stream]),
    'nbasr_frame_signal': (_c_int, [_c_float_p, ctypes.c_void_p, _c_float_p] + [_c_int] * 6 + [_c_stream]),
    'nbasr_power_spectrum': (_c_int, [_c_float_p] * 2 + [_c_int] * 4 + [_c_stream]),
    'nbasr_log_normalize': (_c_int, [_c_float_p, ctypes.c_void_p] + [_c_float_p] * 3 + [_c_int] * 5 + [_c_stream]),
    'nbasr_frontend_stream_state_bytes': (ctypes.c_size_t, [_c_int] * 2),
    'nbasr_frontend_stream_step': (_c_int, [_c_float_p, _c_int, ctypes.c_longlong, _c_float_p, _c_int, _c_int, _c_float_p, _c_int] + [_c_float_p] * 5
                                   + [_c_int] * 4 + [ctypes.c_longlong] + [_c_int] * 6 + [_c_stream]),
    'nbasr_resample_state_bytes': (ctypes.c_size_t, [_c_int] * 2),
    'nbasr_resample_stream_step': (_c_int, [_c_float_p, _c_int, ctypes.c_longlong, _c_float_p, _c_int, _c_int, _c_float_p, _c_int, _c_int, _c_float_p,
                                            _c_int, _c_int, _c_float_p, _c_int, _c_int, ctypes.c_longlong, _c_int, ctypes.c_longlong, _c_int, _c_int,
                                            _c_stream]),
    'nbasr_resample': (_c_int, [_c_float_p, _c_int, _c_int, ctypes.c_void_p, _c_float_p, _c_int, _c_int, _c_float_p] + [_c_int] * 3 + [_c_stream]),
})


def frame_signal(wave, lengths, frames, win, hop):
    """wave (B, L) -> frames (B, win, ld): centred, reflect-padded analysis frames, sample-in-window major."""
    b, ld_wave = wave.shape
    _call('nbasr_frame_signal', _dev(wave, 'wave'), _lengths_ptr(lengths, b), _dev(frames, 'frames'), b, ld_wave, ld_wave, win, hop,
          frames.shape[2], _stream(wave))
    return frames


def pointwise_linear(x, frames, weight, bias, y):
    """y (B, c_out, ld_out) = weight (c_out, c_in) . x (B, c_in, ld_in) + bias, no activation."""
    b, c_in, ld_in = x.shape
    _call('nbasr_pointwise_linear', _dev(x, 'x'), _dev(weight, 'weight'), _dev(bias, 'bias'), _dev(y, 'y'), b, c_in, frames, ld_in,
          weight.shape[0], y.shape[2], _stream(x))
    return y


def power_spectrum(spec, bins, power):
    b, _, ld = spec.shape
    _call('nbasr_power_spectrum', _dev(spec, 'spec'), _dev(power, 'power'), b, bins, power.shape[1], ld, _stream(spec))
    return power


def log_normalize(mel, lengths, mean, inv_scale, feats, samples, hop):
    b, n_mels, ld = mel.shape
    _call('nbasr_log_normalize', _dev(mel, 'mel'), _lengths_ptr(lengths, b), _dev(mean, 'mean'), _dev(inv_scale, 'inv_scale'),
          _dev(feats, 'feats'), b, samples, hop, n_mels, ld, _stream(mel))
    return feats


def frontend_stream_state_bytes(batch, win):
    """Bytes of the two sample tails of a front-end stream (nbasr.h: nbasr_frontend_stream_state_bytes); 0 for bad sizes."""
    return int(load_library().nbasr_frontend_stream_state_bytes(batch, win))


def _wave_rows(wave, b, device, who, check_dtype=True):
    """(samples, row pitch) of a (b, samples) float32 chunk whose rows are contiguous and do not overlap.  ``check_dtype`` False: the
    caller refuses another dtype itself, after this (``frontend_stream_step``, in its own order and words)."""
    shape = wave.shape if isinstance(wave, torch.Tensor) else ()
    if len(shape) != 2 or shape[0] != b or wave.device != device:
        raise HipError(f'{who}: wave must be a ({b}, samples) tensor on {device}')
    n = shape[1]
    if not n:
        return 0, 0
    if check_dtype and wave.dtype != torch.float32:
        raise HipError(f'{who}: wave must be float32 (got {wave.dtype})')
    pitch = wave.stride(0)
    if wave.stride(1) != 1 or (b > 1 and pitch < n):
        raise HipError(f'{who}: the samples of an utterance must be contiguous, the utterances must not overlap')
    return n, max(pitch, n)


def _tail_pair(tail_in, tail_out, samples, who):
    """The batch of a stream step's two tails: (B, round_up4(samples)) tensors, ``tail_out`` possibly None."""
    b, tail_ld = tail_in.shape
    if tail_ld != round_up4(samples) or (tail_out is not None and tuple(tail_out.shape) != (b, tail_ld)):
        raise HipError(f'{who}: the tails must be ({b}, {round_up4(samples)}) tensors')
    return b


def frontend_stream_step(tail_in, tail_len, tail_first, wave, tail_out, tail_out_first_rel, dft_image, fbank_image, mean, inv_scale, feats,
                         col0, first_frame, n_frames, final, win, hop, bins):
    """One step of a front-end stream (nbasr.h: nbasr_frontend_stream_step).  ``tail_in`` / ``tail_out``: (B, round_up4(win + 1)) float32
    tails (``tail_out`` None: retain nothing); ``wave`` (B, n) float32 or None; ``feats`` (B, n_mels, ld) receives frames ``first_frame`` ..
    at columns ``col0`` .. (None when ``n_frames`` is 0).  Returns ``feats``."""
    b = _tail_pair(tail_in, tail_out, win + 1, 'frontend_stream_step')
    n_new, ld_wave = (0, 0) if wave is None else _wave_rows(wave, b, tail_in.device, 'frontend_stream_step', check_dtype=False)
    if n_new and wave.dtype != torch.float32:
        raise HipError(f'wave must be float32 (got {wave.dtype})')
    n_mels = mean.numel()
    ld_feats = 0
    if n_frames:
        if feats.dim() != 3 or feats.shape[0] != b or feats.shape[1] != n_mels or feats.device != tail_in.device:
            raise HipError(f'frontend_stream_step: feats must be a ({b}, {n_mels}, ld) tensor on {tail_in.device}')
        ld_feats = feats.shape[2]
    _call('nbasr_frontend_stream_step', _dev(tail_in, 'tail_in'), int(tail_len), int(tail_first), wave.data_ptr() if n_new else None, n_new,
          ld_wave, _opt(tail_out, 'tail_out'), int(tail_out_first_rel), _dev(dft_image, 'dft_image'), _dev(fbank_image, 'fbank_image'),
          _dev(mean, 'mean'), _dev(inv_scale, 'inv_scale'), _dev(feats, 'feats') if n_frames else None, ld_feats, int(col0), int(first_frame),
          int(n_frames), int(tail_first) + int(tail_len) + n_new, int(bool(final)), b, win, hop, bins, n_mels, _stream(tail_in))
    return feats


def resample_state_bytes(batch, tail_capacity):
    """Bytes of the two sample tails of a resampler stream (nbasr.h: nbasr_resample_state_bytes); 0 for bad sizes."""
    return int(load_library().nbasr_resample_state_bytes(batch, tail_capacity))


def resample_stream_step(tail_in, tail_len, tail_first, wave, tail_out, tail_out_first_rel, tail_capacity, table, orig_freq, new_freq, out,
                         col0, first_out, n_out, final):
    """One step of a resampler stream (nbasr.h: nbasr_resample_stream_step).  ``tail_in`` / ``tail_out``: (B, round_up4(tail_capacity))
    float32 tails (``tail_out`` None: retain nothing); ``wave`` (B, n) float32 or None; ``out`` (B, ld) receives outputs ``first_out`` ..
    at columns ``col0`` .. (None when ``n_out`` is 0).  Returns ``out``."""
    b = _tail_pair(tail_in, tail_out, tail_capacity, 'resample_stream_step')
    n_new, ld_wave = (0, 0) if wave is None else _wave_rows(wave, b, tail_in.device, 'resample_stream_step')
    ld_out = 0
    if n_out:
        if out.dim() != 2 or out.shape[0] != b or out.device != tail_in.device:
            raise HipError(f'resample_stream_step: out must be a ({b}, ld) tensor on {tail_in.device}')
        ld_out = out.shape[1]
    _call('nbasr_resample_stream_step', _dev(tail_in, 'tail_in'), int(tail_len), int(tail_first), wave.data_ptr() if n_new else None, n_new,
          ld_wave, _opt(tail_out, 'tail_out'), int(tail_out_first_rel), int(tail_capacity), _dev(table, 'table'), int(orig_freq), int(new_freq),
          _dev(out, 'out') if n_out else None, ld_out, int(col0), int(first_out), int(n_out), int(tail_first) + int(tail_len) + n_new,
          int(bool(final)), b, _stream(tail_in))
    return out


def resample(wave, lengths, table, orig_freq, new_freq, out):
    """Whole utterances (nbasr.h: nbasr_resample): ``wave`` (B, samples) float32 -> ``out`` (B, ceil(n samples / o)); ``lengths`` an int32
    device tensor of B sample counts or None.  Returns ``out``."""
    b = wave.shape[0] if isinstance(wave, torch.Tensor) and wave.dim() == 2 else 0
    samples, ld_wave = _wave_rows(wave, b, table.device, 'resample')
    if out.dim() != 2 or out.shape[0] != b or out.device != wave.device:
        raise HipError(f'resample: out must be a ({b}, outputs) tensor on {wave.device}')
    if lengths is not None and (lengths.dtype != torch.int32 or lengths.device != wave.device or lengths.numel() != b or not lengths.is_contiguous()):
        raise HipError(f'resample: lengths must be {b} contiguous int32 values on {wave.device}')
    _call('nbasr_resample', wave.data_ptr() if samples else None, ld_wave, samples, None if lengths is None else lengths.data_ptr(), _dev(table, 'table'),
          int(orig_freq), int(new_freq), _dev(out, 'out') if out.numel() else None, out.shape[1], out.shape[1], b, _stream(table))
    return out
