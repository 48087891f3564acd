"""ctypes binding of libnbasr_hip.so (C ABI declared in include/nbasr.h).

PyTorch is used here only as plumbing: device memory (``tensor.data_ptr()``) and the current HIP
stream.  Every wrapper validates device / dtype / contiguity on the host, passes raw pointers
and sizes, and raises ``HipError`` with the library's message on a non-zero return code.  A wrapper
allocates at most its outputs and scratch; the host algorithms that string wrappers together are next
door (walk.py: the forward; backward.py: the dense and LSTM gradients).  There is NO fallback: a missing
library or a tensor off the HIP device fails loudly (build with ``python -m nb_asr_amd.build``).
"""
import ctypes
import operator
import os
import threading
import pathlib

import torch

LIB_PATH = pathlib.Path(__file__).resolve().parent / 'lib' / 'libnbasr_hip.so'
ABI_VERSION = 6

_c_float_p = ctypes.c_void_p      # device pointers travel as opaque addresses
_c_int = ctypes.c_int
_c_stream = ctypes.c_void_p

class DeferredLN(ctypes.Structure):
    """struct nbasr_deferred_ln: per-frame statistics + affine parameters of a pending LayerNorm."""
    _fields_ = [('stats', ctypes.c_void_p), ('gamma', ctypes.c_void_p), ('beta', ctypes.c_void_p)]


_c_ln_p = ctypes.POINTER(DeferredLN)

# name -> (restype, argtypes); must list every symbol declared in include/nbasr.h
SIGNATURES = {
    'nbasr_version': (_c_int, []),
    'nbasr_build_id': (ctypes.c_char_p, []),
    'nbasr_last_error': (ctypes.c_char_p, []),
    'nbasr_pad_amounts': (_c_int, [_c_int, _c_int, _c_int, ctypes.POINTER(_c_int), ctypes.POINTER(_c_int)]),
    'nbasr_output_frames': (_c_int, [_c_int]),
    'nbasr_stream_create': (_c_int, [ctypes.POINTER(ctypes.c_void_p)]),
    # LayerNorm, statistics, node ops (storage-type generic: a trailing dtype code)
    'nbasr_layernorm_channels': (_c_int, [_c_float_p] * 5 + [_c_int] * 4 + [ctypes.c_float, _c_int, _c_int, _c_stream]),
    'nbasr_channel_stats': (_c_int, [_c_float_p] * 2 + [_c_int] * 4 + [ctypes.c_float, _c_int, _c_stream]),
    'nbasr_grouped_stats_workspace_bytes': (ctypes.c_size_t, [_c_int] * 3),
    'nbasr_grouped_stats_finalize': (_c_int, [_c_float_p] * 2 + [_c_int] * 6 + [ctypes.c_float, _c_stream]),
    'nbasr_grouped_conv1d_node': (_c_int, [_c_float_p] * 7 + [_c_int] * 7 + [_c_ln_p, _c_int, _c_int, _c_float_p, _c_int, _c_int, _c_stream]),
    'nbasr_pack_grouped_weights': (_c_int, [_c_float_p] * 2 + [_c_int] * 3 + [_c_stream]),
    'nbasr_grouped_cell_fits': (_c_int, [_c_int] * 3),
    'nbasr_grouped_cell_fused': (_c_int, [_c_float_p, _c_float_p, _c_float_p, _c_int, _c_int, _c_float_p, _c_float_p, _c_int, _c_int,
                                          _c_float_p, _c_float_p, _c_int, _c_int, _c_int, _c_float_p] + [_c_int] * 5 + [_c_ln_p, _c_float_p, _c_int, _c_stream]),
    'nbasr_grouped_cell_mfma_weights_bytes': (ctypes.c_size_t, [_c_int] * 3),
    'nbasr_grouped_cell_mfma_pack': (_c_int, [_c_float_p] * 2 + [_c_int] * 3 + [_c_stream]),
    'nbasr_grouped_cell_mfma_fits': (_c_int, [_c_int] * 3),
    'nbasr_grouped_cell_mfma': (_c_int, [_c_float_p, _c_float_p, _c_float_p, _c_int, _c_int, _c_float_p, _c_float_p, _c_int, _c_int,
                                         _c_float_p, _c_float_p, _c_int, _c_int, _c_int, _c_float_p] + [_c_int] * 5 + [_c_ln_p, _c_stream]),
    'nbasr_skip_sum': (_c_int, [_c_float_p] * 4 + [_c_int] * 4 + [_c_ln_p, _c_int, _c_int, _c_stream]),
    'nbasr_repitch': (_c_int, [_c_float_p] * 2 + [_c_int] * 5 + [_c_stream]),
    'nbasr_convert': (_c_int, [_c_float_p] * 2 + [ctypes.c_longlong, _c_int, _c_int, _c_stream]),
    # dense convolutions
    'nbasr_dense_conv1d_fused': (_c_int, [_c_float_p] * 7 + [_c_int] * 8 + [_c_ln_p, _c_int, _c_int, _c_stream]),
    'nbasr_packed_dense_weights_bytes': (ctypes.c_size_t, [_c_int] * 5),
    'nbasr_pack_dense_weights': (_c_int, [_c_int] + [_c_float_p] * 2 + [_c_int] * 5 + [_c_stream]),
    'nbasr_dense_conv1d_packed': (_c_int, [_c_int, _c_float_p, _c_int] + [_c_float_p] * 8 + [_c_int] * 10 + [_c_ln_p, _c_float_p, _c_stream]),
    'nbasr_input_range': (_c_int, [_c_float_p] * 2 + [_c_int] * 4 + [_c_stream]),
    'nbasr_split_image_bytes': (ctypes.c_size_t, [_c_int] * 3),
    'nbasr_layernorm_split_image': (_c_int, [_c_float_p] * 6 + [_c_int] * 4 + [ctypes.c_float, _c_stream]),
    'nbasr_split_image_ranged': (_c_int, [_c_float_p] * 3 + [_c_int] * 4 + [_c_stream]),
    'nbasr_bf16_image_bytes': (ctypes.c_size_t, [_c_int] * 3),
    'nbasr_bf16_image': (_c_int, [_c_float_p] * 5 + [_c_int] * 4 + [ctypes.c_float, _c_int, _c_stream]),
    # per-frame linear maps
    'nbasr_pointwise_packed_weights_bytes': (ctypes.c_size_t, [_c_int] * 2),
    'nbasr_pointwise_workspace_bytes': (ctypes.c_size_t, [_c_int] * 3),
    'nbasr_pack_pointwise_weights': (_c_int, [_c_float_p] * 2 + [_c_int] * 2 + [_c_stream]),
    'nbasr_linear_fused_packed': (_c_int, [_c_float_p] * 8 + [_c_int] * 5 + [_c_ln_p, _c_int, _c_int, _c_stream]),
    'nbasr_pointwise_linear': (_c_int, [_c_float_p] * 4 + [_c_int] * 6 + [_c_stream]),
    # LSTM + head
    'nbasr_lstm_input_projection': (_c_int, [_c_float_p] * 5 + [_c_int] * 5 + [_c_ln_p, _c_stream]),
    'nbasr_lstm_input_projection_packed': (_c_int, [_c_float_p] * 6 + [_c_int] * 5 + [_c_ln_p, _c_stream]),
    'nbasr_lstm_input_projection_packed_into': (_c_int, [_c_float_p] * 6 + [_c_int] * 5 + [_c_ln_p, _c_int, _c_int, _c_stream]),
    'nbasr_pointwise_bf16_weights_bytes': (ctypes.c_size_t, [_c_int] * 2),
    'nbasr_pointwise_bf16_workspace_bytes': (ctypes.c_size_t, [_c_int] * 3),
    'nbasr_pack_pointwise_weights_bf16': (_c_int, [_c_float_p] * 2 + [_c_int] * 2 + [_c_stream]),
    'nbasr_linear_fused_bf16': (_c_int, [_c_float_p] * 8 + [_c_int] * 5 + [_c_ln_p, _c_int, _c_int, _c_stream]),
    'nbasr_lstm_input_projection_bf16': (_c_int, [_c_float_p] * 6 + [_c_int] * 5 + [_c_ln_p, _c_stream]),
    'nbasr_lstm_packed_whh_bytes': (ctypes.c_size_t, [_c_int]),
    'nbasr_lstm_pack_whh': (_c_int, [_c_float_p] * 2 + [_c_int, _c_stream]),
    'nbasr_lstm_recurrence_packed': (_c_int, [_c_float_p] * 4 + [_c_int] * 3 + [_c_stream]),
    'nbasr_lstm_seq_workspace_bytes': (ctypes.c_size_t, [_c_int] * 2),
    'nbasr_lstm_recurrence_seq': (_c_int, [_c_float_p] * 5 + [_c_int] * 4 + [_c_stream]),
    'nbasr_lstm_seq_status': (_c_int, [_c_float_p, _c_stream]),
    'nbasr_lstm_packed_whh16_bytes': (ctypes.c_size_t, [_c_int]),
    'nbasr_lstm_pack_whh16': (_c_int, [_c_float_p] * 2 + [_c_int, _c_stream]),
    'nbasr_lstm_xcd_workspace_bytes': (ctypes.c_size_t, [_c_int] * 2),
    'nbasr_lstm_recurrence_xcd': (_c_int, [_c_float_p] * 5 + [_c_int] * 4 + [_c_stream]),
    'nbasr_lstm_recurrence_frames16': (_c_int, [_c_float_p] * 5 + [_c_int] * 3 + [_c_stream]),
    'nbasr_lstm_recurrence_frames16_state': (_c_int, [_c_float_p] * 6 + [_c_int] * 4 + [_c_stream]),
    'nbasr_linear_head': (_c_int, [_c_float_p] * 4 + [_c_int] * 3 + [_c_stream]),
    'nbasr_linear_head_bct': (_c_int, [_c_float_p] * 4 + [_c_int] * 5 + [_c_ln_p, _c_stream]),
    # post-logits step
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
    'nbasr_ctc_endpoint_state_bytes': (ctypes.c_size_t, [_c_int]),
    'nbasr_ctc_endpoint_step': (_c_int, [_c_float_p] * 5 + [_c_int, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_float, ctypes.c_void_p]
                                + [_c_int] * 3 + [_c_stream]),
    'nbasr_ctc_segment_state_bytes': (ctypes.c_size_t, [_c_int, _c_int]),
    'nbasr_ctc_segment_step': (_c_int, [_c_float_p] * 4 + [_c_int] * 4 + [ctypes.c_longlong, ctypes.c_longlong, ctypes.c_float, ctypes.c_void_p]
                               + [_c_int] * 3 + [_c_stream]),
    'nbasr_ctc_keyword_state_bytes': (ctypes.c_size_t, [_c_int, _c_int]),
    'nbasr_ctc_keyword_step': (_c_int, [_c_float_p] * 5 + [_c_int] * 2 + [_c_float_p] * 4 + [_c_int] * 3 + [_c_stream]),
    # streaming windows
    'nbasr_stream_window': (_c_int, [_c_float_p] + [_c_int] * 3 + [_c_float_p] + [_c_int] * 3 + [_c_float_p] + [_c_int] * 3 + [_c_float_p, _c_stream]),
    # front-end
    'nbasr_frame_signal': (_c_int, [_c_float_p, ctypes.c_void_p, _c_float_p] + [_c_int] * 6 + [_c_stream]),
    'nbasr_power_spectrum': (_c_int, [_c_float_p] * 2 + [_c_int] * 4 + [_c_stream]),
    'nbasr_log_normalize': (_c_int, [_c_float_p, ctypes.c_void_p] + [_c_float_p] * 3 + [_c_int] * 5 + [_c_stream]),
    'nbasr_frontend_stream_state_bytes': (ctypes.c_size_t, [_c_int] * 2),
    'nbasr_frontend_stream_step': (_c_int, [_c_float_p, _c_int, ctypes.c_longlong, _c_float_p, _c_int, _c_int, _c_float_p, _c_int] + [_c_float_p] * 5
                                   + [_c_int] * 4 + [ctypes.c_longlong] + [_c_int] * 6 + [_c_stream]),
    # resampler
    'nbasr_resample_state_bytes': (ctypes.c_size_t, [_c_int] * 2),
    'nbasr_resample_stream_step': (_c_int, [_c_float_p, _c_int, ctypes.c_longlong, _c_float_p, _c_int, _c_int, _c_float_p, _c_int, _c_int, _c_float_p,
                                            _c_int, _c_int, _c_float_p, _c_int, _c_int, ctypes.c_longlong, _c_int, ctypes.c_longlong, _c_int, _c_int,
                                            _c_stream]),
    'nbasr_resample': (_c_int, [_c_float_p, _c_int, _c_int, ctypes.c_void_p, _c_float_p, _c_int, _c_int, _c_float_p] + [_c_int] * 3 + [_c_stream]),
    # optimisation step
    'nbasr_optim_table_bytes': (ctypes.c_size_t, [_c_int] * 2),
    'nbasr_optim_workspace_bytes': (ctypes.c_size_t, [_c_int] * 2),
    'nbasr_optim_adam_step': (_c_int, [ctypes.c_void_p, _c_int, _c_int, ctypes.c_void_p, _c_float_p] + [ctypes.c_double] * 5 + [_c_stream]),
    # backward building blocks
    'nbasr_grouped_conv1d_backward_workspace_bytes': (ctypes.c_size_t, [_c_int] * 4),
    'nbasr_grouped_conv1d_backward': (_c_int, [_c_float_p] * 8 + [_c_int] * 7 + [_c_stream]),
    'nbasr_layernorm_backward_workspace_bytes': (ctypes.c_size_t, [_c_int] * 3),
    'nbasr_layernorm_channels_backward': (_c_int, [_c_float_p] * 8 + [_c_int] * 4 + [_c_stream]),
    'nbasr_relu_clamp_backward': (_c_int, [_c_float_p] * 3 + [ctypes.c_longlong, _c_stream]),
    'nbasr_zero_stuff': (_c_int, [_c_float_p] * 2 + [_c_int] * 7 + [_c_stream]),
    'nbasr_conv_fold': (_c_int, [_c_float_p] * 2 + [_c_int] * 8 + [_c_stream]),
    'nbasr_dense_conv1d_linear': (_c_int, [_c_float_p] * 4 + [_c_int] * 8 + [_c_stream]),
    'nbasr_conv_cols': (_c_int, [_c_float_p] * 2 + [_c_int] * 10 + [_c_stream]),
    'nbasr_rows_of_channels': (_c_int, [_c_float_p] * 2 + [_c_int] * 5 + [_c_stream]),
    'nbasr_lstm_gate_scan': (_c_int, [_c_float_p] * 2 + [_c_int] * 4 + [_c_stream]),
    'nbasr_lstm_backward_step': (_c_int, [_c_float_p] * 6 + [_c_int] * 5 + [_c_stream]),
}

# entry points that only answer on the host (never recorded on a launch tape); every other one enqueues work on a stream
_HOST_ONLY = frozenset({'nbasr_version', 'nbasr_build_id', 'nbasr_last_error', 'nbasr_pad_amounts', 'nbasr_output_frames', 'nbasr_stream_create',
                        'nbasr_grouped_cell_fits', 'nbasr_grouped_cell_mfma_fits'})
_ENQUEUES = frozenset(name for name in SIGNATURES if name not in _HOST_ONLY and not name.endswith('_bytes')
                      and '_bytes_' not in name)

F32, BF16 = 0, 1                 # NBASR_F32 / NBASR_BF16
GC_FPL8, GC_WPERM, GC_OSPLIT, GC_PIPE, GC_RING = 1, 2, 4, 8, 16         # NBASR_GC_* variant bits of nbasr_grouped_conv1d_node


class HipError(RuntimeError):
    """``code``: the entry point's return value (a negative NBASR_E* argument error or a positive hipError_t), None for errors raised
    on the python side."""
    code = None


_lib = None
_tls = threading.local()


class _TapingLibrary:
    """Stand-in for the loaded library while a ``ForwardPlan`` records a launch tape (tape.LaunchTape): every entry
    point that takes a stream -- i.e. enqueues work -- is executed AND appended to ``entries`` as ``[function, [args]]``;
    host-only queries (sizes, error text, version) pass straight through."""

    def __init__(self, lib, entries):
        self._lib, self._entries = lib, entries

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name not in _ENQUEUES:
            return fn
        entries = self._entries

        def call(*args):
            entries.append([fn, list(args)])
            return fn(*args)
        return call


def start_tape(entries):
    """Record this thread's enqueueing library calls into ``entries`` until ``stop_tape()``."""
    _tls.taping = _TapingLibrary(load_library(), entries)


def stop_tape():
    _tls.taping = None


def load_library(path=None):
    """Load (once) and type the shared library.  Raises if it has not been built."""
    global _lib
    if path is None:
        taping = getattr(_tls, 'taping', None)
        if taping is not None:
            return taping
        if _lib is not None:
            return _lib
    p = pathlib.Path(path) if path is not None else LIB_PATH
    if not p.exists():
        raise HipError(f'{p} not found: the HIP extension has not been built '
                       f'(run `python -m nb_asr_amd.build`); there is no CPU fallback')
    lib = ctypes.CDLL(str(p))
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(lib, name)        # AttributeError if a declared symbol is not exported
        fn.restype = restype
        fn.argtypes = argtypes
    got = lib.nbasr_version()
    if got != ABI_VERSION:
        raise HipError(f'{p}: ABI version {got}, binding expects {ABI_VERSION}; rebuild the library')
    if path is None:
        _lib = lib
    return lib


def build_id():
    """Build id compiled into the loaded library (see ``nb_asr_amd.build.source_hash``)."""
    return load_library().nbasr_build_id().decode('ascii', 'replace')


def _check(rc, what):
    if rc != 0:
        msg = load_library().nbasr_last_error().decode('utf-8', 'replace')
        err = HipError(f'{what} failed with code {rc}: {msg}')
        err.code = int(rc)
        raise err


def _stream(t):
    return torch.cuda.current_stream(t.device).cuda_stream


def _dev(t, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise HipError(f'{name} must be a tensor on a HIP device (got {getattr(t, "device", type(t))}); '
                       f'this package has no CPU path')
    if t.dtype != torch.float32:
        raise HipError(f'{name} must be float32 (got {t.dtype})')
    if not t.is_contiguous():
        raise HipError(f'{name} must be contiguous')
    return t.data_ptr()


def _opt(t, name):
    return None if t is None else _dev(t, name)


def dtype_code(dtype):
    if dtype == torch.float32:
        return F32
    if dtype == torch.bfloat16:
        return BF16
    raise HipError(f'activations must be float32 or bfloat16 (got {dtype})')


def row_pitch(frames, dtype=torch.float32):
    """Row pitch of an activation tensor: whole 16-byte chunks (4 fp32 / 8 bf16 frames)."""
    return (frames + 7) & ~7 if dtype == torch.bfloat16 else (frames + 3) & ~3


def _act(t, name, dtype=None):
    """Device pointer of an activation tensor of either storage type (float32 / bfloat16), contiguous."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise HipError(f'{name} must be a tensor on a HIP device (got {getattr(t, "device", type(t))}); '
                       f'this package has no CPU path')
    if t.dtype not in (torch.float32, torch.bfloat16) or (dtype is not None and t.dtype != dtype):
        raise HipError(f'{name} must be {dtype or "float32 or bfloat16"} (got {t.dtype})')
    if not t.is_contiguous():
        raise HipError(f'{name} must be contiguous')
    return t.data_ptr()


def _act_opt(t, name, dtype):
    return None if t is None else _act(t, name, dtype)


def _ln(ln):
    """(stats, gamma, beta) tensors of a pending LayerNorm -> pointer to a nbasr_deferred_ln (or NULL)."""
    if ln is None:
        return None
    stats, gamma, beta = ln
    return ctypes.byref(DeferredLN(_dev(stats, 'ln.stats'), _dev(gamma, 'ln.gamma'), _dev(beta, 'ln.beta')))


# ---------------------------------------------------------------------------------------------
# host-only helpers (usable without a GPU)
# ---------------------------------------------------------------------------------------------
def pad_amounts(kernel, dilation, stride):
    left, right = _c_int(), _c_int()
    _check(load_library().nbasr_pad_amounts(kernel, dilation, stride, ctypes.byref(left), ctypes.byref(right)),
           'nbasr_pad_amounts')
    return left.value, right.value


def output_frames(frames):
    return load_library().nbasr_output_frames(frames)


def round_up4(n):
    return (n + 3) & ~3


def dense_mode():
    """NBASR_DENSE_MODE as it is set NOW, validated; the one place that reads it.  Dense k = 8 convs, fp32-accurate in every mode: 'auto' (default)
    = 2-way fp16 split (3 MFMAs per product) wherever the input has just been written by the LayerNorm kernel (which also emits the per-utterance
    max|x| its range scaling needs), else the 3-way bf16 split (6 MFMAs, fp32's exponent range); 'bf16x3' = that everywhere; 'f32' = exact-fp32 MFMA."""
    mode = os.environ.get('NBASR_DENSE_MODE', 'auto')
    if mode not in ('auto', 'bf16x3', 'f32'):
        raise ValueError(f'NBASR_DENSE_MODE must be auto, bf16x3 or f32, got {mode!r}')
    return mode


def _skips3(skips):
    return list(skips) + [None] * (3 - len(skips))


# ---------------------------------------------------------------------------------------------
# device entry points; activations are (batch, channels, ld) float32 tensors whose last dimension
# is the row pitch ld (a multiple of 4) and `frames` <= ld the number of valid frames
# ---------------------------------------------------------------------------------------------
def grouped_conv1d_fused(x, weight, bias, skips, y, frames, groups, kernel, dilation, ln=None, ln_on_x=False,
                         ln_on_skip0=False, stats_out=None, stats_ws=None, eps=0.0):
    """The fp32 node op (the default kernel of grouped_conv1d_node).  `ln` = (stats, gamma, beta) of a pending LayerNorm carried by x
    (ln_on_x) and/or skips[0] (ln_on_skip0).  `stats_ws` (grouped_stats_workspace): also emit the partial LayerNorm statistics of y;
    with `stats_out` (B, 2, ld) they are merged at once (grouped_stats_finalize)."""
    if stats_out is not None and stats_ws is None:
        raise HipError('grouped_conv1d_fused: stats_out needs the partial-statistics workspace stats_ws')
    grouped_conv1d_node(x, weight, bias, skips, y, frames, groups, kernel, dilation, ln, ln_on_x, ln_on_skip0, stats_ws, 0)
    if stats_out is not None and x.shape[0] and x.shape[2]:
        grouped_stats_finalize(stats_ws, stats_out, x.shape[1], frames, groups, eps)
    return y


def grouped_cell_fits(channels, ld, groups):
    """0 when a (channels, ld, groups) cell cannot run as one launch, else the groups per statistics partial of that launch (4 or 2)."""
    return int(load_library().nbasr_grouped_cell_fits(channels, ld, groups))


def grouped_cell_fused(x0, nodes, skip_mask, y, frames, groups, ln=None, stats_ws=None):
    """nodes: three (weight, bias, kernel, dilation), ``weight`` = the [group][ci][tap][co] copy of ``pack_grouped_weights`` (ABI 4);
    skip_mask: bit0 s00 | bit1 s10 | bit2 s11 | bit3 s20 | bit4 s21 | bit5 s22.
    ``stats_ws`` (grouped_stats_workspace): also emit the partial LayerNorm statistics of the result (merge: grouped_stats_finalize)."""
    b, c, ld = x0.shape
    args = []
    for w, bias, k, d in nodes:
        args += [_dev(w, 'weight'), _dev(bias, 'bias'), k, d]
    dtype = x0.dtype
    _check(load_library().nbasr_grouped_cell_fused(_act(x0, 'x0', dtype), *args, skip_mask, _act(y, 'y', dtype), b, c, frames, ld, groups,
                                                   _ln(ln), _opt(stats_ws, 'stats_ws'), dtype_code(dtype), _stream(x0)), 'nbasr_grouped_cell_fused')
    return y


def grouped_cell_mfma_fits(channels, ld, groups):
    """0 when a bf16 (channels, ld, groups) cell cannot run as one matrix-core launch, else its groups per workgroup."""
    return int(load_library().nbasr_grouped_cell_mfma_fits(channels, ld, groups))


def grouped_cell_mfma_pack(weight, groups):
    """(C, C/groups, k) fp32 weight (the values of a bf16 parameter) -> the MFMA fragment image grouped_cell_mfma takes for that node."""
    c, _, k = weight.shape
    nbytes = load_library().nbasr_grouped_cell_mfma_weights_bytes(c, groups, k)
    if nbytes == 0:
        raise HipError(f'grouped_cell_mfma_pack: weight shape {tuple(weight.shape)} with {groups} groups is not a node op of the search space')
    packed = torch.empty(nbytes, dtype=torch.uint8, device=weight.device)
    _check(load_library().nbasr_grouped_cell_mfma_pack(_dev(weight, 'weight'), packed.data_ptr(), c, groups, k, _stream(weight)),
           'nbasr_grouped_cell_mfma_pack')
    return packed


def grouped_cell_mfma(x0, nodes, skip_mask, y, frames, groups, ln=None):
    """The bf16 cell on the matrix cores.  nodes: three (packed weight from grouped_cell_mfma_pack, fp32 bias, kernel, dilation)."""
    b, c, ld = x0.shape
    args = []
    for packed, bias, k, d in nodes:
        if not packed.is_cuda or packed.dtype != torch.uint8 or packed.numel() != load_library().nbasr_grouped_cell_mfma_weights_bytes(c, groups, k):
            raise HipError('grouped_cell_mfma: node weights must be the uint8 tensors of grouped_cell_mfma_pack for this (channels, groups, kernel)')
        args += [packed.data_ptr(), _dev(bias, 'bias'), k, d]
    _check(load_library().nbasr_grouped_cell_mfma(_act(x0, 'x0', torch.bfloat16), *args, skip_mask, _act(y, 'y', torch.bfloat16), b, c, frames, ld,
                                                  groups, _ln(ln), _stream(x0)), 'nbasr_grouped_cell_mfma')
    return y


def grouped_stats_finalize(stats_ws, stats_out, channels, frames, groups, eps, groups_per_part=4):
    """Merge the partial statistics a node / fused-cell launch left in ``stats_ws`` into (mean, rstd) rows.  ``groups_per_part``: 4 for
    the node kernels, ``grouped_cell_fits(...)`` (4 or 2) for a fused cell."""
    b, _, ld = stats_out.shape
    _check(load_library().nbasr_grouped_stats_finalize(_dev(stats_ws, 'stats_ws'), _dev(stats_out, 'stats_out'), b, channels,
                                                       frames, ld, groups, int(groups_per_part), float(eps), _stream(stats_out)),
           'nbasr_grouped_stats_finalize')
    return stats_out


def grouped_stats_workspace(batch, ld, groups, device):
    n = load_library().nbasr_grouped_stats_workspace_bytes(batch, ld, groups) // 4
    return torch.empty(max(n, 4), dtype=torch.float32, device=device)


def skip_sum(skips, y, frames, ln=None, ln_on_skip0=False):
    """Node whose main op is `zero`: y = sum of the skips (float32 or bfloat16 tensors, all of y's type)."""
    b, c, ld = y.shape
    dt = y.dtype
    s = _skips3(skips)
    _check(load_library().nbasr_skip_sum(_act_opt(s[0], 'skip0', dt), _act_opt(s[1], 'skip1', dt), _act_opt(s[2], 'skip2', dt),
                                         _act(y, 'y'), b, c, frames, ld, _ln(ln), int(ln_on_skip0), dtype_code(dt), _stream(y)),
           'nbasr_skip_sum')
    return y


def channel_stats(x, stats, frames, eps):
    """One read pass over x (B, C, ld), float32 or bfloat16: stats (B, 2, ld) <- per-frame (mean, 1/sqrt(var + eps)) over channels."""
    b, c, ld = x.shape
    _check(load_library().nbasr_channel_stats(_act(x, 'x'), _dev(stats, 'stats'), b, c, frames, ld, float(eps), dtype_code(x.dtype),
                                              _stream(x)), 'nbasr_channel_stats')
    return stats


def layernorm_channels(x, gamma, beta, y, frames, eps, absmax=None):
    """LayerNorm over channels, x -> y (float32 -> float32, bfloat16 -> bfloat16 or bfloat16 -> float32); with ``absmax`` (a (B,)
    float32 device tensor; float32 tensors only) also max|y[b]| per utterance."""
    b, c, ld = x.shape
    if absmax is not None and absmax.numel() != b:
        raise HipError('absmax must hold one float per utterance')
    _check(load_library().nbasr_layernorm_channels(_act(x, 'x'), _dev(gamma, 'gamma'), _dev(beta, 'beta'), _act(y, 'y'),
                                                   _opt(absmax, 'absmax'), b, c, frames, ld, float(eps), dtype_code(x.dtype),
                                                   dtype_code(y.dtype), _stream(x)), 'nbasr_layernorm_channels')
    return y


def split_image(batch, channels, ld, device):
    """Buffer for the pre-split fp16 image of a (batch, channels, ld) activation (layernorm_split_image)."""
    return torch.empty(max(load_library().nbasr_split_image_bytes(batch, channels, ld), 16), dtype=torch.uint8, device=device)


def layernorm_split_image(x, gamma, beta, stats, bound, image, frames, eps):
    """LayerNorm(x) written as the fp16-split image of the dense convolution; also fills stats (B, 2, ld) and bound (B)."""
    b, c, ld = x.shape
    if image.dtype != torch.uint8 or image.numel() < load_library().nbasr_split_image_bytes(b, c, ld):
        raise HipError('image buffer too small: allocate it with split_image(batch, channels, ld, device)')
    _check(load_library().nbasr_layernorm_split_image(_dev(x, 'x'), _dev(gamma, 'gamma'), _dev(beta, 'beta'), _dev(stats, 'stats'),
                                                      _dev(bound, 'bound'), image.data_ptr(), b, c, frames, ld, float(eps), _stream(x)),
           'nbasr_layernorm_split_image')
    return image


def dense_conv1d_fused_packed_f16_img(image, bound, batch, c_in, frames_in, ld_in, packed, c_out, kernel, bias, y, stride,
                                      row_tile=128, stats_part=None, frame_tile=256):
    """The fp16x2 convolution on the pre-split operand image (layernorm_split_image): LDS-DMA-only GEMM.  ``stats_part``: also emit
    the partial LayerNorm statistics of y (dense_stats_part_floats)."""
    _check_packed(packed, 'f16x2', c_out, c_in, kernel, row_tile)
    if image.numel() < load_library().nbasr_split_image_bytes(batch, c_in, ld_in):
        raise HipError('image buffer too small for (batch, c_in, ld_in)')
    return _dense_packed('f16x2', image.data_ptr(), True, bound, None, packed, bias, (None, None, None), y, _dev(y, 'y'), batch, c_in,
                         frames_in, ld_in, c_out, kernel, stride, row_tile, None, _stream(y), stats_part, frame_tile)


def input_range(x, frames, out):
    """out (B, 4) float32 <- per utterance (max finite |x|, quietest non-silent frame's max, non-finite flag, -); see nbasr.h."""
    b, c, ld = x.shape
    if out.numel() < 4 * b:
        raise HipError('input_range: out needs 4 floats per utterance')
    _check(load_library().nbasr_input_range(_dev(x, 'x'), _dev(out, 'range'), b, c, frames, ld, _stream(x)), 'nbasr_input_range')
    return out


def dense_conv1d_first_ranged(x, frames_in, x_range, packed_f16, packed_bf16x3, c_out, kernel, bias, y, stride, image=None, row_tile=128,
                              stats_part=None, frame_tile=256):
    """The model's first dense conv with per-utterance routing on the device: ordinary utterances on the 2-way fp16 split,
    extreme ones (non-finite samples, > 2^12 dynamic range between frames) on the 3-way bf16 split; same output tensor.
    ``image``: uint8 workspace of ``nbasr_split_image_bytes`` -- the fp16 leg then runs on the image path (one split pass over
    x, LDS-DMA-only GEMM; ``packed_f16`` packed for ``row_tile``); None: the input is split in the GEMM's prologue."""
    lib = load_library()
    b, c_in, ld_in = x.shape
    _check_packed(packed_f16, 'f16x2', c_out, c_in, kernel, 128 if image is None else row_tile)
    _check_packed(packed_bf16x3, 'bf16x3', c_out, c_in, kernel)
    none3, stream = (None, None, None), _stream(x)
    if image is not None:
        if image.dtype != torch.uint8 or image.numel() < lib.nbasr_split_image_bytes(b, c_in, ld_in):
            raise HipError('dense_conv1d_first_ranged: image workspace too small (nbasr_split_image_bytes)')
        _check(lib.nbasr_split_image_ranged(_dev(x, 'x'), _dev(x_range, 'x_range'), image.data_ptr(), b, c_in, frames_in, ld_in, stream),
               'nbasr_split_image_ranged')
    if image is not None:
        _dense_packed('f16x2', image.data_ptr(), True, None, x_range, packed_f16, bias, none3, y, _dev(y, 'y'), b, c_in, frames_in, ld_in,
                      c_out, kernel, stride, row_tile, None, stream, stats_part, frame_tile)
    else:
        _dense_packed('f16x2', _dev(x, 'x'), False, None, x_range, packed_f16, bias, none3, y, _dev(y, 'y'), b, c_in, frames_in, ld_in,
                      c_out, kernel, stride, 128, None, stream, stats_part)
    return _dense_packed('bf16x3', _dev(x, 'x'), False, None, x_range, packed_bf16x3, bias, none3, y, _dev(y, 'y'), b, c_in, frames_in,
                         ld_in, c_out, kernel, stride, 128, None, stream, stats_part)


def dense_conv1d_fused(x, frames_in, weight, bias, skips, y, stride, ln=None, ln_on_x=False, ln_on_skip0=False):
    b, c_in, ld_in = x.shape
    c_out, _, kernel = weight.shape if weight.dim() == 3 else (weight.shape[0], weight.shape[1], 1)
    ld_out = y.shape[2]
    s = _skips3(skips)
    _check(load_library().nbasr_dense_conv1d_fused(
        _dev(x, 'x'), _dev(weight, 'weight'), _dev(bias, 'bias'), _opt(s[0], 'skip0'), _opt(s[1], 'skip1'),
        _opt(s[2], 'skip2'), _dev(y, 'y'), b, c_in, frames_in, ld_in, c_out, ld_out, kernel, stride, _ln(ln), int(ln_on_x),
        int(ln_on_skip0), _stream(x)), 'nbasr_dense_conv1d_fused')
    return y


DENSE_SCHEMES = {'bf16x3': 0, 'f16x2': 1, 'bf16': 2}        # NBASR_DENSE_* of nbasr_dense_conv1d_packed


def _scheme_code(scheme):
    if scheme not in DENSE_SCHEMES:
        raise HipError(f"unknown operand scheme {scheme!r} (expected 'bf16x3', 'f16x2' or 'bf16')")
    return DENSE_SCHEMES[scheme]


def packed_dense_weights_bytes(scheme, c_out, c_in, kernel, row_tile=128):
    return load_library().nbasr_packed_dense_weights_bytes(_scheme_code(scheme), c_out, c_in, kernel, row_tile)


def pack_dense_weights(weight, stride, scheme='bf16x3', row_tile=128):
    """(c_out, c_in, 8) fp32 weight -> opaque uint8 tensor holding its operand form (3 x bf16 split, 2 x fp16 split for
    ``scheme='f16x2'``, one bf16 term for 'bf16') in the LDS layout of the stride-`stride` kernel that will consume it.  ``row_tile``
    other than 128: the 64- / 160-row tiles of the image-path kernels (f16x2: 64, 160; bf16: 160)."""
    code = _scheme_code(scheme)
    lib = load_library()
    c_out, c_in, kernel = weight.shape
    nbytes = lib.nbasr_packed_dense_weights_bytes(code, c_out, c_in, kernel, row_tile)
    if nbytes == 0:
        raise HipError(f'packed dense path ({scheme}) does not cover weight shape {tuple(weight.shape)} with row_tile={row_tile}')
    if not weight.is_cuda:
        raise HipError('weight must be on a HIP device')
    packed = torch.empty(nbytes, dtype=torch.uint8, device=weight.device)
    _check(lib.nbasr_pack_dense_weights(code, _dev(weight, 'weight'), packed.data_ptr(), c_out, c_in, kernel, stride, row_tile,
                                        _stream(weight)), 'nbasr_pack_dense_weights')
    packed.nbasr_row_tile = row_tile           # the packed sizes of the two tilings can coincide (c_out = 1200): remember which
    return packed


def _dense_packed(scheme, x_ptr, image, x_absmax, x_range, packed, bias, s, y, y_ptr, b, c_in, frames_in, ld_in, c_out, kernel, stride,
                  row_tile, ln, stream, stats_part=None, frame_tile=256):
    """The one C entry point of the packed k = 8 convolution (nbasr.h: nbasr_dense_conv1d_packed)."""
    if stats_part is not None and stats_part.numel() < dense_stats_part_floats(b, c_out, y.shape[2]):
        raise HipError('stats_part too small: ceil(c_out / 16) * batch * 2 * ld_out floats (dense_stats_part_floats)')
    _check(load_library().nbasr_dense_conv1d_packed(
        _scheme_code(scheme), x_ptr, int(image), _opt(x_absmax, 'x_absmax'), _opt(x_range, 'x_range'), packed.data_ptr(),
        _dev(bias, 'bias'), _opt(s[0], 'skip0'), _opt(s[1], 'skip1'), _opt(s[2], 'skip2'), y_ptr, b, c_in, frames_in, ld_in, c_out,
        y.shape[2], kernel, stride, row_tile, int(frame_tile), _ln(ln), _opt(stats_part, 'stats_part'), stream), 'nbasr_dense_conv1d_packed')
    return y


DENSE_STATS_UNIT = 16         # nbasr.h: NBASR_DENSE_STATS_UNIT


def dense_stats_part_floats(batch, c_out, ld_out):
    """Floats of the statistics partials a dense convolution emits with ``stats_part``: one (mean, M2) row pair per 16 output channels
    (merge: grouped_stats_finalize(part, stats, c_out, frames_out, c_out, eps, DENSE_STATS_UNIT))."""
    return -(-c_out // DENSE_STATS_UNIT) * batch * 2 * ld_out


def _check_packed(packed, scheme, c_out, c_in, kernel, row_tile=128):
    if not packed.is_cuda or packed.dtype != torch.uint8:
        raise HipError('packed weights must be the uint8 device tensor returned by pack_dense_weights')
    if packed.numel() != packed_dense_weights_bytes(scheme, c_out, c_in, kernel, row_tile) or getattr(packed, 'nbasr_row_tile', 128) != row_tile:
        raise HipError(f'packed weights have {packed.numel()} bytes: not a {scheme} image of a ({c_out}, {c_in}, {kernel}) weight for '
                       f'row_tile={row_tile}')


def dense_conv1d_fused_packed(x, frames_in, packed, c_out, kernel, bias, skips, y, stride, ln=None, scheme='bf16x3',
                              x_absmax=None, stats_part=None):
    """Dense k=8 conv on packed weights; ``scheme`` must be the one the weights were packed with.  'f16x2' needs
    ``x_absmax``: a (B,) float32 device tensor of upper bounds of max|x[b]| (see nbasr.h) and takes no deferred LayerNorm.
    ``stats_part`` (no skips): also emit the partial LayerNorm statistics of y (dense_stats_part_floats)."""
    b, c_in, ld_in = x.shape
    s = _skips3(skips)
    _check_packed(packed, scheme, c_out, c_in, kernel)
    if scheme == 'f16x2':
        if ln is not None:
            raise HipError('the f16x2 scheme takes no deferred LayerNorm (it needs the range of the normalised tensor)')
        if x_absmax is None or x_absmax.numel() != b:
            raise HipError('the f16x2 scheme needs x_absmax: one float32 bound of max|x[b]| per utterance')
    elif ln is not None and any(t is not None for t in s):
        raise HipError('the packed path takes a deferred LayerNorm only without skip inputs')
    return _dense_packed(scheme, _dev(x, 'x'), False, x_absmax if scheme == 'f16x2' else None, None, packed, bias, s, y, _dev(y, 'y'),
                         b, c_in, frames_in, ld_in, c_out, kernel, stride, 128, ln, _stream(x), stats_part)


def lstm_forward(x, frames, w_ih, w_hh, b_ih, b_hh, gates_ws, cell_ws, h_out, ln=None):
    """nn.LSTM forward as its two library calls on one stream: the exact-fp32 input projection, then the per-frame recurrence."""
    lstm_input_projection(x, frames, w_ih, b_ih, b_hh, gates_ws, w_hh.shape[1], ln)
    return lstm_recurrence(gates_ws, w_hh, cell_ws, h_out)


def lstm_input_projection(x, frames, w_ih, b_ih, b_hh, gates_ws, hidden, ln=None):
    """gates_ws (frames, batch, 4*hidden) <- x . w_ih^T + b_ih + b_hh for all frames (first half of lstm_forward)."""
    b, c_in, ld = x.shape
    _check(load_library().nbasr_lstm_input_projection(
        _dev(x, 'x'), _dev(w_ih, 'w_ih'), _dev(b_ih, 'b_ih'), _dev(b_hh, 'b_hh'), _dev(gates_ws, 'gates_ws'),
        b, c_in, frames, ld, hidden, _ln(ln), _stream(x)), 'nbasr_lstm_input_projection')
    return gates_ws


def lstm_pack_whh(w_hh):
    """(4H, H) recurrent weight -> opaque uint8 tensor in the operand-fragment order of the step kernel."""
    hidden = w_hh.shape[1]
    packed = torch.empty(load_library().nbasr_lstm_packed_whh_bytes(hidden), dtype=torch.uint8, device=w_hh.device)
    _check(load_library().nbasr_lstm_pack_whh(_dev(w_hh, 'w_hh'), packed.data_ptr(), hidden, _stream(w_hh)), 'nbasr_lstm_pack_whh')
    return packed


def _check_whh(packed_whh, h_out):
    hidden = h_out.shape[2]
    if not packed_whh.is_cuda or packed_whh.dtype != torch.uint8 or packed_whh.numel() != load_library().nbasr_lstm_packed_whh_bytes(hidden):
        raise HipError('packed_whh must be the uint8 device tensor returned by lstm_pack_whh for this hidden size')
    return h_out.shape


def lstm_recurrence_packed(gates_ws, packed_whh, cell_ws, h_out):
    b, frames, hidden = _check_whh(packed_whh, h_out)
    _check(load_library().nbasr_lstm_recurrence_packed(_dev(gates_ws, 'gates_ws'), packed_whh.data_ptr(), _dev(cell_ws, 'cell_ws'),
                                                       _dev(h_out, 'h_out'), b, frames, hidden, _stream(h_out)),
           'nbasr_lstm_recurrence_packed')
    return h_out


def lstm_seq_workspace(batch, hidden, device):
    """Workspace of the one-launch recurrence (flags + the exchange images of h), or None where that form does not apply."""
    nbytes = lstm_seq_workspace_bytes(int(batch), int(hidden), device)
    return torch.empty(nbytes, dtype=torch.uint8, device=device) if nbytes else None


HIP_ERROR_COOPERATIVE_LAUNCH_TOO_LARGE = 720       # hipErrorCooperativeLaunchTooLarge: nbasr_lstm_recurrence_seq passes a refused grid's code through
LSTM_SEQ_INJECT_FAULT = 1       # NBASR_LSTM_SEQ_INJECT_FAULT of nbasr_lstm_recurrence_seq (tests)
LSTM_CONTINUE = 2               # NBASR_LSTM_CONTINUE of nbasr_lstm_recurrence_frames16_state


def lstm_recurrence_seq(gates_ws, packed_whh, cell_ws, h_out, seq_ws, flags=0):
    """lstm_recurrence_packed with all frames in ONE (cooperative) launch: w_hh resident in registers, h exchanged in payload-tagged
    granules; same h_out, bit for bit.  The first int32 of ``seq_ws`` is the status word (non-zero: a step timed out, h_out holds NaN)."""
    b, frames, hidden = _check_whh(packed_whh, h_out)
    need = lstm_seq_workspace_bytes(b, hidden, h_out.device)
    if need == 0 or seq_ws is None or not seq_ws.is_cuda or seq_ws.dtype != torch.uint8 or seq_ws.numel() < need:
        raise HipError(f'lstm_recurrence_seq: batch={b} hidden={hidden} needs a uint8 device workspace of {need} bytes from lstm_seq_workspace '
                       '(0 = this form does not apply)')
    _check(load_library().nbasr_lstm_recurrence_seq(_dev(gates_ws, 'gates_ws'), packed_whh.data_ptr(), _dev(cell_ws, 'cell_ws'), _dev(h_out, 'h_out'),
                                                    seq_ws.data_ptr(), b, frames, hidden, int(flags), _stream(h_out)), 'nbasr_lstm_recurrence_seq')
    return h_out


def lstm_seq_workspace_bytes(batch, hidden, device):
    """Workspace of the one-launch recurrence on ``device`` (0: that form does not apply there).  The answer depends on how many
    workgroups THAT device holds at once, and the C query asks the current device: it runs with ``device`` current."""
    with torch.cuda.device(device):
        return load_library().nbasr_lstm_seq_workspace_bytes(batch, hidden)


def lstm_seq_status(seq_ws):
    """Synchronises the current stream and raises HipError if a step of the last one-launch recurrence timed out."""
    _check(load_library().nbasr_lstm_seq_status(seq_ws.data_ptr(), _stream(seq_ws)), 'nbasr_lstm_seq_status')


def lstm_pack_whh16(w_hh):
    """w_hh (4*hidden, hidden) fp32 -> the resident operand image of lstm_recurrence_xcd (two fp16 terms per weight; hidden <= 512)."""
    hidden = w_hh.shape[1]
    lib = load_library()
    nbytes = lib.nbasr_lstm_packed_whh16_bytes(hidden)
    if w_hh.shape[0] != 4 * hidden or nbytes == 0:
        raise HipError(f'lstm_pack_whh16: w_hh must be (4*hidden, hidden) with hidden <= 512, got {tuple(w_hh.shape)}')
    packed = torch.empty(nbytes, dtype=torch.uint8, device=w_hh.device)
    _check(lib.nbasr_lstm_pack_whh16(_dev(w_hh, 'w_hh'), packed.data_ptr(), hidden, _stream(w_hh)), 'nbasr_lstm_pack_whh16')
    return packed


def lstm_xcd_workspace_bytes(batch, hidden):
    return load_library().nbasr_lstm_xcd_workspace_bytes(int(batch), int(hidden))


def lstm_xcd_workspace(batch, hidden, device):
    nbytes = lstm_xcd_workspace_bytes(batch, hidden)
    if nbytes == 0:
        raise HipError(f'lstm_recurrence_xcd does not apply to batch={batch}, hidden={hidden} (hidden <= 512, batch <= 4096)')
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def _check_whh16(packed_whh16, xcd_ws, h_out, who, hint=''):
    batch, _, hidden = h_out.shape
    if not packed_whh16.is_cuda or packed_whh16.dtype != torch.uint8 or packed_whh16.numel() != load_library().nbasr_lstm_packed_whh16_bytes(hidden):
        raise HipError('packed_whh16 must be the uint8 device tensor returned by lstm_pack_whh16 for this hidden size')
    need = lstm_xcd_workspace_bytes(batch, hidden)
    if need == 0 or not xcd_ws.is_cuda or xcd_ws.dtype != torch.uint8 or xcd_ws.numel() < need:
        raise HipError(f'{who}: batch={batch} hidden={hidden} needs a uint8 device workspace of {need} bytes from lstm_xcd_workspace{hint}')
    return h_out.shape


def lstm_recurrence_xcd(gates_ws, packed_whh16, cell_ws, h_out, xcd_ws, flags=0):
    """The recurrence as ONE resident launch, a tile of 16 utterances per XCD, on the fp16 matrix cores (nbasr.h, ABI 6): h_out agrees
    with lstm_recurrence_packed to fp32 round-off.  The status word of ``xcd_ws`` is read by ``lstm_seq_status``."""
    b, frames, hidden = _check_whh16(packed_whh16, xcd_ws, h_out, 'lstm_recurrence_xcd', ' (0 = the form does not apply)')
    _check(load_library().nbasr_lstm_recurrence_xcd(_dev(gates_ws, 'gates_ws'), packed_whh16.data_ptr(), _dev(cell_ws, 'cell_ws'), _dev(h_out, 'h_out'),
                                                    xcd_ws.data_ptr(), b, frames, hidden, int(flags), _stream(h_out)), 'nbasr_lstm_recurrence_xcd')
    return h_out


def lstm_recurrence_frames16(gates_ws, packed_whh16, cell_ws, h_out, xcd_ws):
    """lstm_recurrence_xcd's arithmetic as one launch per frame (bit-identical h_out): the form of a pipelined tail and of a demoted plan."""
    b, frames, hidden = _check_whh16(packed_whh16, xcd_ws, h_out, 'lstm_recurrence_frames16')
    _check(load_library().nbasr_lstm_recurrence_frames16(_dev(gates_ws, 'gates_ws'), packed_whh16.data_ptr(), _dev(cell_ws, 'cell_ws'), _dev(h_out, 'h_out'),
                                                         xcd_ws.data_ptr(), b, frames, hidden, _stream(h_out)), 'nbasr_lstm_recurrence_frames16')
    return h_out


def lstm_recurrence_frames16_state(gates_ws, packed_whh16, cell_ws, h_out, xcd_ws, h0=None, flags=0):
    """lstm_recurrence_frames16 with carried state: ``flags=LSTM_CONTINUE`` starts frame 0 from c = ``cell_ws`` and h = ``h0``
    ((batch, hidden) float32, None = zeros) instead of zeros (nbasr.h).  flags = 0 and h0 = None: bit-identical to lstm_recurrence_frames16."""
    b, frames, hidden = _check_whh16(packed_whh16, xcd_ws, h_out, 'lstm_recurrence_frames16_state')
    if h0 is not None and h0.numel() != b * hidden:
        raise HipError(f'lstm_recurrence_frames16_state: h0 must hold ({b}, {hidden}) floats')
    _check(load_library().nbasr_lstm_recurrence_frames16_state(_dev(gates_ws, 'gates_ws'), packed_whh16.data_ptr(), _dev(cell_ws, 'cell_ws'),
                                                               _dev(h_out, 'h_out'), xcd_ws.data_ptr(), _opt(h0, 'h0'), b, frames, hidden,
                                                               int(flags), _stream(h_out)), 'nbasr_lstm_recurrence_frames16_state')
    return h_out


def lstm_recurrence(gates_ws, w_hh, cell_ws, h_out):
    """h_out (batch, frames, hidden) from the projected gates (second half of lstm_forward), on the current stream; packs w_hh per call
    (a caller that keeps the weight packs it once: lstm_pack_whh + lstm_recurrence_packed)."""
    return lstm_recurrence_packed(gates_ws, lstm_pack_whh(w_hh), cell_ws, h_out)


def pack_pointwise_weights(weight):
    """(c_out, c_in) fp32 weight of a per-frame linear map -> opaque uint8 tensor (2 x fp16 split in LDS-image order + row scales)."""
    c_out, c_in = weight.shape
    nbytes = load_library().nbasr_pointwise_packed_weights_bytes(c_out, c_in)
    packed = torch.empty(nbytes, dtype=torch.uint8, device=weight.device)
    _check(load_library().nbasr_pack_pointwise_weights(_dev(weight, 'weight'), packed.data_ptr(), c_out, c_in, _stream(weight)),
           'nbasr_pack_pointwise_weights')
    return packed


def pointwise_workspace(batch, c_in, ld, device):
    """Scratch for the pre-split activation image of linear_fused_packed / lstm_input_projection_packed."""
    return torch.empty(max(load_library().nbasr_pointwise_workspace_bytes(batch, c_in, ld), 16), dtype=torch.uint8, device=device)


def _check_pointwise(packed, ws, c_out, c_in, batch, ld):
    lib = load_library()
    if not packed.is_cuda or packed.dtype != torch.uint8 or packed.numel() != lib.nbasr_pointwise_packed_weights_bytes(c_out, c_in):
        raise HipError(f'packed weights are not the pack_pointwise_weights image of a ({c_out}, {c_in}) weight')
    if not ws.is_cuda or ws.dtype != torch.uint8 or ws.numel() < lib.nbasr_pointwise_workspace_bytes(batch, c_in, ld):
        raise HipError('workspace too small: allocate it with pointwise_workspace(batch, c_in, ld, device)')


def linear_fused_packed(x, frames, packed, c_out, bias, skips, y, ws, ln=None, ln_on_x=False, ln_on_skip0=False):
    """The `linear` node op on the fp16 matrix cores: y = min(relu(W x + b), 20) + skips (see nbasr.h)."""
    b, c_in, ld = x.shape
    _check_pointwise(packed, ws, c_out, c_in, b, ld)
    s = _skips3(skips)
    _check(load_library().nbasr_linear_fused_packed(
        _dev(x, 'x'), ws.data_ptr(), packed.data_ptr(), _dev(bias, 'bias'), _opt(s[0], 'skip0'), _opt(s[1], 'skip1'),
        _opt(s[2], 'skip2'), _dev(y, 'y'), b, c_in, frames, ld, c_out, _ln(ln), int(ln_on_x), int(ln_on_skip0), _stream(x)),
        'nbasr_linear_fused_packed')
    return y


def lstm_input_projection_packed(x, frames, packed_w_ih, b_ih, b_hh, gates_ws, hidden, ws, ln=None, batch_total=None, batch_offset=0):
    """``batch_total``: gates_ws is the (frames, batch_total, 4 hidden) gate tensor of SEVERAL forwards and this call fills utterances
    batch_offset .. batch_offset + batch - 1 of it (one recurrence over all of them follows: nbasr.h)."""
    b, c_in, ld = x.shape
    _check_pointwise(packed_w_ih, ws, 4 * hidden, c_in, b, ld)
    if batch_total is not None:
        if gates_ws.numel() < frames * batch_total * 4 * hidden:
            raise HipError(f'lstm_input_projection_packed: gates_ws holds {gates_ws.numel()} floats, ({frames}, {batch_total}, {4 * hidden}) needs more')
        _check(load_library().nbasr_lstm_input_projection_packed_into(
            _dev(x, 'x'), ws.data_ptr(), packed_w_ih.data_ptr(), _dev(b_ih, 'b_ih'), _dev(b_hh, 'b_hh'), _dev(gates_ws, 'gates_ws'),
            b, c_in, frames, ld, hidden, _ln(ln), batch_total, batch_offset, _stream(x)), 'nbasr_lstm_input_projection_packed_into')
        return gates_ws
    _check(load_library().nbasr_lstm_input_projection_packed(
        _dev(x, 'x'), ws.data_ptr(), packed_w_ih.data_ptr(), _dev(b_ih, 'b_ih'), _dev(b_hh, 'b_hh'), _dev(gates_ws, 'gates_ws'),
        b, c_in, frames, ld, hidden, _ln(ln), _stream(x)), 'nbasr_lstm_input_projection_packed')
    return gates_ws


def pack_pointwise_weights_bf16(weight):
    """(c_out, c_in) fp32 values of a bf16 weight -> opaque uint8 tensor (bf16, LDS-image order) for the bf16 per-frame maps."""
    c_out, c_in = weight.shape
    packed = torch.empty(load_library().nbasr_pointwise_bf16_weights_bytes(c_out, c_in), dtype=torch.uint8, device=weight.device)
    _check(load_library().nbasr_pack_pointwise_weights_bf16(_dev(weight, 'weight'), packed.data_ptr(), c_out, c_in, _stream(weight)),
           'nbasr_pack_pointwise_weights_bf16')
    return packed


def pointwise_bf16_workspace(batch, c_in, ld, device):
    return torch.empty(max(load_library().nbasr_pointwise_bf16_workspace_bytes(batch, c_in, ld), 16), dtype=torch.uint8, device=device)


def _check_pointwise_bf16(packed, ws, c_out, c_in, batch, ld):
    lib = load_library()
    if not packed.is_cuda or packed.dtype != torch.uint8 or packed.numel() != lib.nbasr_pointwise_bf16_weights_bytes(c_out, c_in):
        raise HipError(f'packed weights are not the pack_pointwise_weights_bf16 image of a ({c_out}, {c_in}) weight')
    if not ws.is_cuda or ws.dtype != torch.uint8 or ws.numel() < lib.nbasr_pointwise_bf16_workspace_bytes(batch, c_in, ld):
        raise HipError('workspace too small: allocate it with pointwise_bf16_workspace(batch, c_in, ld, device)')


def linear_fused_bf16(x, frames, packed, c_out, bias, skips, y, ws, ln=None, ln_on_x=False, ln_on_skip0=False):
    """The `linear` node op on bf16 rows, one bf16 MFMA per product: y = bf16(min(relu(W x + b), 20) + skips) (see nbasr.h)."""
    b, c_in, ld = x.shape
    bf = torch.bfloat16
    _check_pointwise_bf16(packed, ws, c_out, c_in, b, ld)
    s = _skips3(skips)
    _check(load_library().nbasr_linear_fused_bf16(
        _act(x, 'x', bf), ws.data_ptr(), packed.data_ptr(), _dev(bias, 'bias'), _act_opt(s[0], 'skip0', bf), _act_opt(s[1], 'skip1', bf),
        _act_opt(s[2], 'skip2', bf), _act(y, 'y', bf), b, c_in, frames, ld, c_out, _ln(ln), int(ln_on_x), int(ln_on_skip0), _stream(x)),
        'nbasr_linear_fused_bf16')
    return y


def lstm_input_projection_bf16(x, frames, packed_w_ih, b_ih, b_hh, gates_ws, hidden, ws, ln=None):
    """gates (frames, batch, 4 hidden) fp32 from the bf16 encoder output x (batch, c_in, ld), its pending LayerNorm applied on the way."""
    b, c_in, ld = x.shape
    _check_pointwise_bf16(packed_w_ih, ws, 4 * hidden, c_in, b, ld)
    _check(load_library().nbasr_lstm_input_projection_bf16(
        _act(x, 'x', torch.bfloat16), ws.data_ptr(), packed_w_ih.data_ptr(), _dev(b_ih, 'b_ih'), _dev(b_hh, 'b_hh'), _dev(gates_ws, 'gates_ws'),
        b, c_in, frames, ld, hidden, _ln(ln), _stream(x)), 'nbasr_lstm_input_projection_bf16')
    return gates_ws


def _lengths_ptr(lengths, batch):
    if lengths is None:
        return None
    if not lengths.is_cuda or lengths.dtype != torch.int32 or not lengths.is_contiguous() or lengths.numel() != batch:
        raise HipError('lengths must be a contiguous int32 device tensor with one entry per utterance')
    return lengths.data_ptr()


def frame_signal(wave, lengths, frames, win, hop):
    """wave (B, L) -> frames (B, win, ld): centred, reflect-padded analysis frames, sample-in-window major."""
    b, ld_wave = wave.shape
    _check(load_library().nbasr_frame_signal(_dev(wave, 'wave'), _lengths_ptr(lengths, b), _dev(frames, 'frames'), b, ld_wave,
                                             ld_wave, win, hop, frames.shape[2], _stream(wave)), 'nbasr_frame_signal')
    return frames


def pointwise_linear(x, frames, weight, bias, y):
    """y (B, c_out, ld_out) = weight (c_out, c_in) . x (B, c_in, ld_in) + bias, no activation."""
    b, c_in, ld_in = x.shape
    _check(load_library().nbasr_pointwise_linear(_dev(x, 'x'), _dev(weight, 'weight'), _dev(bias, 'bias'), _dev(y, 'y'), b, c_in,
                                                 frames, ld_in, weight.shape[0], y.shape[2], _stream(x)), 'nbasr_pointwise_linear')
    return y


def power_spectrum(spec, bins, power):
    b, _, ld = spec.shape
    _check(load_library().nbasr_power_spectrum(_dev(spec, 'spec'), _dev(power, 'power'), b, bins, power.shape[1], ld, _stream(spec)),
           'nbasr_power_spectrum')
    return power


def log_normalize(mel, lengths, mean, inv_scale, feats, samples, hop):
    b, n_mels, ld = mel.shape
    _check(load_library().nbasr_log_normalize(_dev(mel, 'mel'), _lengths_ptr(lengths, b), _dev(mean, 'mean'),
                                              _dev(inv_scale, 'inv_scale'), _dev(feats, 'feats'), b, samples, hop, n_mels, ld,
                                              _stream(mel)), 'nbasr_log_normalize')
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
    _check(load_library().nbasr_frontend_stream_step(
        _dev(tail_in, 'tail_in'), int(tail_len), int(tail_first), wave.data_ptr() if n_new else None, n_new, ld_wave,
        _opt(tail_out, 'tail_out'), int(tail_out_first_rel), _dev(dft_image, 'dft_image'), _dev(fbank_image, 'fbank_image'), _dev(mean, 'mean'),
        _dev(inv_scale, 'inv_scale'), _dev(feats, 'feats') if n_frames else None, ld_feats, int(col0), int(first_frame), int(n_frames),
        int(tail_first) + int(tail_len) + n_new, int(bool(final)), b, win, hop, bins, n_mels, _stream(tail_in)), 'nbasr_frontend_stream_step')
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
    _check(load_library().nbasr_resample_stream_step(
        _dev(tail_in, 'tail_in'), int(tail_len), int(tail_first), wave.data_ptr() if n_new else None, n_new, ld_wave,
        _opt(tail_out, 'tail_out'), int(tail_out_first_rel), int(tail_capacity), _dev(table, 'table'), int(orig_freq), int(new_freq),
        _dev(out, 'out') if n_out else None, ld_out, int(col0), int(first_out), int(n_out), int(tail_first) + int(tail_len) + n_new,
        int(bool(final)), b, _stream(tail_in)), 'nbasr_resample_stream_step')
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
    _check(load_library().nbasr_resample(
        wave.data_ptr() if samples else None, ld_wave, samples, None if lengths is None else lengths.data_ptr(), _dev(table, 'table'),
        int(orig_freq), int(new_freq), _dev(out, 'out') if out.numel() else None, out.shape[1], out.shape[1], b, _stream(table)), 'nbasr_resample')
    return out


def linear_head(h, weight, bias, logits):
    classes, features = weight.shape
    rows = h.numel() // features
    _check(load_library().nbasr_linear_head(_dev(h, 'h'), _dev(weight, 'weight'), _dev(bias, 'bias'),
                                            _dev(logits, 'logits'), rows, features, classes, _stream(h)),
           'nbasr_linear_head')
    return logits


def linear_head_bct(x, frames, weight, bias, logits, ln=None):
    b, features, ld = x.shape
    classes = weight.shape[0]
    _check(load_library().nbasr_linear_head_bct(_dev(x, 'x'), _dev(weight, 'weight'), _dev(bias, 'bias'),
                                                _dev(logits, 'logits'), b, features, frames, ld, classes, _ln(ln),
                                                _stream(x)), 'nbasr_linear_head_bct')
    return logits


def repitch(src, dst, frames):
    """src (..., ld_src) -> dst (..., ld_dst), float32 or bfloat16: copy `frames` columns, zero the rest of dst's pitch."""
    rows = src.numel() // src.shape[-1]
    _check(load_library().nbasr_repitch(_act(src, 'src'), _act(dst, 'dst', src.dtype), rows, frames, src.shape[-1], dst.shape[-1],
                                        dtype_code(src.dtype), _stream(src)), 'nbasr_repitch')
    return dst


def ctc_postprocess(logits, lengths=None, want_log_probs=True, want_tokens=True, blank=0):
    """logits (B, T', C) -> (log_probs or None, tokens (B, T') int32 padded with -1 or None, token_counts (B) or None)."""
    _dev(logits, 'logits')
    b, t, c = logits.shape
    log_probs = torch.empty_like(logits) if want_log_probs else None
    tokens = torch.empty(b, t, dtype=torch.int32, device=logits.device) if want_tokens else None
    counts = torch.empty(b, dtype=torch.int32, device=logits.device) if want_tokens else None
    _check(load_library().nbasr_ctc_postprocess(
        logits.data_ptr(), _lengths_ptr(lengths, b), None if log_probs is None else log_probs.data_ptr(),
        None if tokens is None else tokens.data_ptr(), None if counts is None else counts.data_ptr(), b, t, c, blank,
        _stream(logits)), 'nbasr_ctc_postprocess')
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
    _check(load_library().nbasr_ctc_greedy_stream(logits.data_ptr() if t else None, prev.data_ptr(), tokens.data_ptr() if t else None,
                                                  counts.data_ptr(), b, t, c, blank, _stream(logits)), 'nbasr_ctc_greedy_stream')
    return tokens, counts


def stream_window(hist, hist_off, n_hist, src, src_off, n_new, dst, absmax=None):
    """One stage window of a streaming session (nbasr.h: nbasr_stream_window).  ``hist`` / ``src`` / ``dst``: (batch, channels, ld)
    float32 tensors with their own row pitches (``hist`` / ``src`` may be None when their frame count is 0); ``absmax`` (batch) or None."""
    b, c, dst_ld = dst.shape
    for t, what in ((hist, 'hist'), (src, 'src')):
        if t is not None and (t.shape[0] != b or t.shape[1] != c):
            raise HipError(f'stream_window: {what} has shape {tuple(t.shape)}, dst {tuple(dst.shape)}')
    if absmax is not None and absmax.numel() != b:
        raise HipError('stream_window: absmax must hold one float per utterance')
    _check(load_library().nbasr_stream_window(
        _opt(hist, 'hist') if n_hist else None, hist.shape[2] if hist is not None else 0, int(hist_off), int(n_hist),
        _opt(src, 'src') if n_new else None, src.shape[2] if src is not None else 0, int(src_off), int(n_new),
        _dev(dst, 'dst'), dst_ld, b, c, _opt(absmax, 'absmax'), _stream(dst)), 'nbasr_stream_window')
    return dst


def _int_tensor(t, what, device, shape=None):
    if not t.is_cuda or t.device != device or t.dtype != torch.int32 or not t.is_contiguous():
        raise HipError(f'{what} must be a contiguous int32 tensor on {device}')
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise HipError(f'{what} must have shape {tuple(shape)}, got {tuple(t.shape)}')
    return t


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
# the same, ready for a call: the picker of the arguments is built once, here
_BEAM_PICKERS = {key: (name, operator.itemgetter(*names)) for key, (name, names) in BEAM_ENTRY_POINTS.items()}


def _beam_call(lib, op, timesteps, fused, values):
    """One call of the entry point of ``BEAM_ENTRY_POINTS`` for (op, timesteps, fused), its arguments picked from ``values`` by name (a
    fused, untimed call passes NULL for the timed-only outputs)."""
    name, pick = _BEAM_PICKERS[op, bool(timesteps), fused]
    _check(getattr(lib, name)(*pick(values)), name)


def _ptr(t):
    return None if t is None else t.data_ptr()


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
    if state.device != dev or state.numel() * state.element_size() < ctc_beam_stream_state_bytes(b, beam_width, pool_nodes, timesteps):
        raise HipError(f'{who}: state must be a tensor of ctc_beam_stream_state_bytes bytes on the device of log_probs')
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
    ws = torch.empty((max(ws_bytes(b, t, c, beam_width), 8) + 7) // 8, dtype=torch.int64, device=dev)   # rounded UP: B * T' * C floats may be odd
    _beam_call(lib, 'search', timesteps, fusion is not None, {
        'log_probs': log_probs.data_ptr(), 'lengths': _ptr(lengths), 'fusion': _ptr(fusion), 'ws': ws.data_ptr(), 'beams': beams.data_ptr(),
        'scores': scores.data_ptr(), 'timesteps': _ptr(steps), 'beam_lens': lens.data_ptr(), 'batch': b, 'frames': t, 'classes': c,
        'beam_width': beam_width, 'blank': blank, 'cutoff_top_n': cutoff_top_n, 'timed': 1 if timesteps else 0, 'stream': _stream(log_probs)})
    return beam_result(*outs)


def ctc_beam_stream_state_bytes(batch, beam_width, pool_nodes, timesteps=False):
    """Bytes of the state of a streaming beam search (nbasr.h: nbasr_ctc_beam_stream_state_bytes, or _timed_state_bytes); 0 for bad sizes."""
    lib = load_library()
    fn = lib.nbasr_ctc_beam_stream_timed_state_bytes if timesteps else lib.nbasr_ctc_beam_stream_state_bytes
    return int(fn(batch, beam_width, pool_nodes))


def _state(state, what='state'):
    if not isinstance(state, torch.Tensor) or not state.is_cuda or not state.is_contiguous():
        raise HipError(f'{what} must be a contiguous tensor on a HIP device')
    return state.data_ptr()


def ctc_beam_stream_init(state, batch, beam_width, pool_nodes, timesteps=False):
    """Every utterance of ``state`` (a device tensor of ``ctc_beam_stream_state_bytes`` bytes) to the empty prefix."""
    if state.numel() * state.element_size() < ctc_beam_stream_state_bytes(batch, beam_width, pool_nodes, timesteps):
        raise HipError('ctc_beam_stream_init: state tensor too small (ctc_beam_stream_state_bytes)')
    _beam_call(load_library(), 'init', timesteps, False,
               {'state': _state(state), 'batch': batch, 'beam_width': beam_width, 'pool_nodes': pool_nodes, 'stream': _stream(state)})


def ctc_beam_stream_step(log_probs, chunk_lengths, state, beam_width, pool_nodes, blank=0, cutoff_top_n=40, timesteps=False, fusion=None):
    """One chunk of a streaming beam search (nbasr.h: nbasr_ctc_beam_stream_step): log_probs (B, n, C) float32, chunk_lengths (B)
    int32 device tensor or None.  Returns device tensors (committed (B, pool_nodes), partial (B, pool_nodes), counts (3, B) int32 =
    committed counts, partial counts, pool usage (-1: refused, the pool is too small for this chunk)).  ``timesteps`` (a state of the
    timed family, nbasr_ctc_beam_stream_timed_step): (committed, partial, committed_frames, partial_frames, counts).  ``fusion``: as
    ``ctc_beam_search`` takes it (nbasr_ctc_beam_stream_lm_step, over a state of either family)."""
    b, t, c, dev = _check_stream_chunk('ctc_beam_stream_step', log_probs, chunk_lengths, fusion, state, beam_width, pool_nodes, timesteps)
    rows = torch.empty(4 if timesteps else 2, b, pool_nodes, dtype=torch.int32, device=dev).unbind(0)
    counts = torch.empty(3, b, dtype=torch.int32, device=dev)
    lib = load_library()
    ws = torch.empty(max(lib.nbasr_ctc_beam_stream_workspace_bytes(b, t, c, pool_nodes), 8) // 4 + 1, dtype=torch.int32, device=dev)
    count_ptr = counts.data_ptr()                              # its rows: committed counts, partial counts, usage, 4 * b bytes each
    _beam_call(lib, 'step', timesteps, fusion is not None, {
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
    _beam_call(load_library(), 'finish', timesteps, False, {
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
        ws = torch.empty((max(need, 8) + 7) // 8, dtype=torch.int64, device=dev)
    elif ws.device != dev or not ws.is_contiguous() or ws.numel() * ws.element_size() < need:
        raise HipError(f'ctc_beam_stream_peek: the workspace must be a contiguous tensor of {need} bytes on {dev}')
    beams, scores, steps, lens = outs = _beam_outputs(b, beam_width, max(int(ld), 1), timesteps, dev)
    _beam_call(load_library(), 'peek', timesteps, fusion is not None, {
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
    _check(load_library().nbasr_token_error_counts(
        hyp.data_ptr(), hyp_len.data_ptr(), hyp.shape[1], ref.data_ptr(), ref_len.data_ptr(), ref.shape[1],
        None if table is None else table.data_ptr(), 0 if table is None else table.numel(), blank, counts.data_ptr(), b,
        torch.cuda.current_stream(dev).cuda_stream), 'nbasr_token_error_counts')
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
    _check(load_library().nbasr_ctc_loss(log_probs.data_ptr(), lengths.data_ptr(), targets.data_ptr(), target_lengths.data_ptr(),
                                         losses.data_ptr(), b, t, c, targets.shape[1], blank, 1 if divide_by_length else 0,
                                         _stream(log_probs)), 'nbasr_ctc_loss')
    return losses


def ctc_loss_grad(log_probs, lengths, targets, target_lengths, blank=0):
    """-> (per-utterance loss / length (B), d mean(loss / length) / d logits (B, T', C)) for log_probs = log_softmax(logits)."""
    b, t, c, dev = _ctc_args(log_probs, lengths, targets, target_lengths)
    losses = torch.empty(b, dtype=torch.float32, device=dev)
    grad = torch.empty_like(log_probs)
    ws = torch.empty(max(load_library().nbasr_ctc_grad_workspace_bytes(b, t, targets.shape[1]) // 4, 1), dtype=torch.float32, device=dev)
    _check(load_library().nbasr_ctc_loss_grad(log_probs.data_ptr(), lengths.data_ptr(), targets.data_ptr(), target_lengths.data_ptr(), ws.data_ptr(),
                                              losses.data_ptr(), grad.data_ptr(), b, t, c, targets.shape[1], blank, _stream(log_probs)), 'nbasr_ctc_loss_grad')
    return losses, grad


def ctc_forced_align(log_probs, lengths, targets, target_lengths, blank=0):
    """The best CTC path of each transcript (nbasr.h: nbasr_ctc_forced_align; arguments as ``ctc_loss``) -> (scores (B) float32,
    path (B, T') int32, starts (B, L) int32, ends (B, L) int32, token_scores (B, L) float32)."""
    b, t, c, dev = _ctc_args(log_probs, lengths, targets, target_lengths)
    ld = targets.shape[1]
    lib = load_library()
    scores = torch.empty(b, dtype=torch.float32, device=dev)
    path = torch.empty(b, t, dtype=torch.int32, device=dev)
    starts, ends = torch.empty(b, ld, dtype=torch.int32, device=dev), torch.empty(b, ld, dtype=torch.int32, device=dev)
    token_scores = torch.empty(b, ld, dtype=torch.float32, device=dev)
    ws = torch.empty(max(lib.nbasr_ctc_align_workspace_bytes(b, t, ld) // 4, 1), dtype=torch.int32, device=dev)
    _check(lib.nbasr_ctc_forced_align(log_probs.data_ptr(), lengths.data_ptr(), targets.data_ptr(), target_lengths.data_ptr(), ws.data_ptr(),
                                      scores.data_ptr(), path.data_ptr(), starts.data_ptr(), ends.data_ptr(), token_scores.data_ptr(),
                                      b, t, c, ld, blank, _stream(log_probs)), 'nbasr_ctc_forced_align')
    return scores, path, starts, ends, token_scores


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
    """One step of the endpointer (nbasr.h: nbasr_ctc_endpoint_step) over ``x`` (B, n, C) float32 logits or log-probabilities.
    ``lengths``: int32 device tensor (B) or None.  ``state_in`` / ``state_out``: (B, 8) int32 device tensors -- ``state_in`` None starts
    fresh rows, the same tensor twice commits in place, two tensors leave ``state_in`` as it was.  ``rules``: (n_rules, 3) int32 device
    table; ``speech_lo`` / ``speech_hi``: the class mask's two 64-bit words; ``mask_out``: (B, n) uint8 device tensor or None.
    Returns ``state_out``."""
    b, n, c = _detector_step_args('ctc_endpoint_step', x, lengths, state_in, state_out, ENDPOINT_STATE_WORDS)
    _int_tensor(rules, 'rules', x.device, (rules.shape[0], 3))
    _check(load_library().nbasr_ctc_endpoint_step(
        x.data_ptr() if x.numel() else None, None if lengths is None else lengths.data_ptr(), None if state_in is None else state_in.data_ptr(),
        state_out.data_ptr(), rules.data_ptr(), rules.shape[0], _signed64(speech_lo), _signed64(speech_hi), float(margin),
        _speech_mask_arg('ctc_endpoint_step', mask_out, x), b, n, c, _stream(x)), 'nbasr_ctc_endpoint_step')
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
    """One step of the segmenter (nbasr.h: nbasr_ctc_segment_step) over ``x`` (B, n, C) float32 logits or log-probabilities.
    ``lengths``: int32 device tensor (B) or None.  ``state_in`` / ``state_out``: (B, 8 + 4 capacity) int32 device tensors -- ``state_in``
    None starts fresh rows, the same tensor twice commits in place, two tensors leave ``state_in`` as it was.  ``min_speech``,
    ``min_silence``, ``max_frames``, ``capacity``: the counts, by value; ``speech_lo`` / ``speech_hi``: the class mask's two 64-bit
    words; ``mask_out``: (B, n) uint8 device tensor or None.  Returns ``state_out``."""
    capacity = int(capacity)
    if not 1 <= capacity <= SEGMENT_MAX_CAPACITY:
        raise HipError(f'ctc_segment_step: capacity={capacity} must lie in [1, {SEGMENT_MAX_CAPACITY}]')
    b, n, c = _detector_step_args('ctc_segment_step', x, lengths, state_in, state_out, ctc_segment_state_words(capacity))
    _check(load_library().nbasr_ctc_segment_step(
        x.data_ptr() if x.numel() else None, None if lengths is None else lengths.data_ptr(), None if state_in is None else state_in.data_ptr(),
        state_out.data_ptr(), int(min_speech), int(min_silence), int(max_frames), capacity, _signed64(speech_lo), _signed64(speech_hi),
        float(margin), _speech_mask_arg('ctc_segment_step', mask_out, x), b, n, c, _stream(x)), 'nbasr_ctc_segment_step')
    return state_out


KEYWORD_STATE_WORDS = 136        # 32-bit words per (utterance, keyword): frames, hit (frame, start, score), best (frame, start, score), 0, V[64], start[64]
KEYWORD_MAX_TOKENS = 32          # the pitch of the token table


def ctc_keyword_state_bytes(batch, n_keywords):
    """Bytes of the keyword state of ``batch`` utterances and ``n_keywords`` keywords (nbasr.h: nbasr_ctc_keyword_state_bytes); 0 when
    either is not positive."""
    return int(load_library().nbasr_ctc_keyword_state_bytes(int(batch), int(n_keywords)))


def ctc_keyword_step(x, lengths, tokens, token_counts, thresholds, blank, state_in, state_out, scores_out=None, starts_out=None):
    """One step of the keyword spotter (nbasr.h: nbasr_ctc_keyword_step) over ``x`` (B, n, C) float32 logits or log-probabilities.
    ``lengths``: int32 device tensor (B) or None.  ``tokens``: (K, 32) int32 device table, -1 past a keyword's end; ``token_counts``:
    (K) int32; ``thresholds``: (K) float32.  ``state_in`` / ``state_out``: (B, K, 136) int32 device tensors -- ``state_in`` None starts
    fresh rows, the same tensor twice commits in place, two tensors leave ``state_in`` as it was.  ``scores_out`` / ``starts_out``:
    (B, K, n) float32 / int32 device tensors, both or neither.  Returns ``state_out``."""
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
    _check(load_library().nbasr_ctc_keyword_step(
        x.data_ptr() if x.numel() else None, None if lengths is None else lengths.data_ptr(), tokens.data_ptr(), token_counts.data_ptr(),
        thresholds.data_ptr(), k, int(blank), None if state_in is None else state_in.data_ptr(), state_out.data_ptr(),
        scores_out.data_ptr() if trace else None, starts_out.data_ptr() if trace else None, b, n, c, _stream(x)), 'nbasr_ctc_keyword_step')
    return state_out


# ---------------------------------------------------------------------------------------------
# storage-type generic entry points (float32 | bfloat16 activations; SURVEY 8 row g1 / BASELINE config 4)
# ---------------------------------------------------------------------------------------------
def pack_grouped_weights(weight, groups):
    """(C, C/groups, k) fp32 weight -> [group][ci][tap][co] copy for the GC_WPERM kernel variants."""
    c, cg, k = weight.shape
    packed = torch.empty_like(weight)
    _check(load_library().nbasr_pack_grouped_weights(_dev(weight, 'weight'), _dev(packed, 'packed'), c, groups, k, _stream(weight)),
           'nbasr_pack_grouped_weights')
    return packed


def grouped_conv1d_node(x, weight, bias, skips, y, frames, groups, kernel, dilation, ln=None, ln_on_x=False, ln_on_skip0=False,
                        stats_ws=None, variant=0):
    """The grouped-conv node op for float32 or bfloat16 activations; ``weight`` / ``bias`` are float32 (``weight`` in the
    layout the variant wants: torch's, or pack_grouped_weights' for GC_WPERM)."""
    b, c, ld = x.shape
    dt = x.dtype
    s = _skips3(skips)
    _check(load_library().nbasr_grouped_conv1d_node(
        _act(x, 'x'), _dev(weight, 'weight'), _dev(bias, 'bias'), _act_opt(s[0], 'skip0', dt), _act_opt(s[1], 'skip1', dt),
        _act_opt(s[2], 'skip2', dt), _act(y, 'y', dt), b, c, frames, ld, groups, kernel, dilation, _ln(ln), int(ln_on_x),
        int(ln_on_skip0), _opt(stats_ws, 'stats_ws'), dtype_code(dt), variant, _stream(x)), 'nbasr_grouped_conv1d_node')
    return y


def convert(x, y):
    """Storage conversion float32 <-> bfloat16 of equally shaped contiguous tensors (numel % 8 == 0)."""
    if x.shape != y.shape:
        raise HipError('convert: shapes differ')
    _check(load_library().nbasr_convert(_act(x, 'x'), _act(y, 'y'), x.numel(), dtype_code(x.dtype), dtype_code(y.dtype), _stream(x)),
           'nbasr_convert')
    return y


def bf16_image_bytes(batch, channels, ld):
    return load_library().nbasr_bf16_image_bytes(batch, channels, ld)


def bf16_image(x, image, frames, norm=None, stats=None, eps=0.0):
    """Operand image of the bf16 dense conv from x (B, C, ld); ``norm`` = (gamma, beta): image of LayerNorm(x), ``stats`` filled."""
    b, c, ld = x.shape
    if image.dtype != torch.uint8 or image.numel() < bf16_image_bytes(b, c, ld):
        raise HipError('image buffer too small: needs bf16_image_bytes(batch, channels, ld) bytes of uint8')
    gamma, beta = norm if norm is not None else (None, None)
    _check(load_library().nbasr_bf16_image(_act(x, 'x'), _opt(gamma, 'gamma'), _opt(beta, 'beta'), _opt(stats, 'stats'),
                                           image.data_ptr(), b, c, frames, ld, float(eps), dtype_code(x.dtype), _stream(x)),
           'nbasr_bf16_image')
    return image


def pack_dense_weights_bf16(weight, stride, row_tile=128):
    """(c_out, c_in, 8) fp32 weight (the values of a bf16 parameter) -> packed one-term bf16 image of the stride-`stride` kernel."""
    return pack_dense_weights(weight, stride, 'bf16', row_tile)


def dense_conv1d_bf16_img(image, batch, c_in, frames_in, ld_in, packed, c_out, kernel, bias, y, stride, row_tile=128, frame_tile=256):
    _check_packed(packed, 'bf16', c_out, c_in, kernel, row_tile)
    if image.numel() < load_library().nbasr_bf16_image_bytes(batch, c_in, ld_in):
        raise HipError('image buffer too small for (batch, c_in, ld_in)')
    return _dense_packed('bf16', image.data_ptr(), True, None, None, packed, bias, (None, None, None), y, _act(y, 'y', torch.bfloat16), batch,
                         c_in, frames_in, ld_in, c_out, kernel, stride, row_tile, None, _stream(y), None, frame_tile)


# ---------------------------------------------------------------------------------------------
# backward building blocks; backward.py strings the last eight together (nbasr.h says what each computes)
# ---------------------------------------------------------------------------------------------
def grouped_conv1d_backward(x, weight, z, dz, frames, groups, kernel, dilation, need_dx=True, need_dw=True):
    """Gradients of z = min(relu(grouped_conv(x, weight) + bias), 20) given dz: (dx or None, dw or None, db or None).
    x, z, dz: (B, C, ld) float32 pitched tensors (z = the op's output; dz's pitch columns zero)."""
    b, c, ld = z.shape
    lib = load_library()
    dx = torch.empty_like(z) if need_dx else None
    dw = torch.empty_like(weight) if need_dw else None
    db = torch.empty(c, dtype=torch.float32, device=z.device) if need_dw else None
    ws = None
    if need_dw:
        ws = torch.empty(max(lib.nbasr_grouped_conv1d_backward_workspace_bytes(max(b, 1), c, groups, kernel) // 4, 4), dtype=torch.float32,
                         device=z.device)
    _check(lib.nbasr_grouped_conv1d_backward(_opt(x, 'x'), _dev(weight, 'weight'), _dev(z, 'z'), _dev(dz, 'dz'), _opt(dx, 'dx'), _opt(dw, 'dw'),
                                             _opt(db, 'db'), _opt(ws, 'workspace'), b, c, frames, ld, groups, kernel, dilation, _stream(z)),
           'nbasr_grouped_conv1d_backward')
    return dx, dw, db


def layernorm_channels_backward(x, stats, gamma, dy, frames):
    """(dx, dgamma, dbeta) of y = LayerNorm_channels(x) given dy; stats = channel_stats(x)."""
    b, c, ld = x.shape
    lib = load_library()
    dx = torch.empty_like(x)
    dgamma = torch.empty(c, dtype=torch.float32, device=x.device)
    dbeta = torch.empty(c, dtype=torch.float32, device=x.device)
    ws = torch.empty(max(lib.nbasr_layernorm_backward_workspace_bytes(max(b, 1), c, max(ld, 4)) // 4, 4), dtype=torch.float32, device=x.device)
    _check(lib.nbasr_layernorm_channels_backward(_dev(x, 'x'), _dev(stats, 'stats'), _dev(gamma, 'gamma'), _dev(dy, 'dy'), _dev(dx, 'dx'),
                                                 _dev(dgamma, 'dgamma'), _dev(dbeta, 'dbeta'), _dev(ws, 'workspace'), b, c, frames, ld, _stream(x)),
           'nbasr_layernorm_channels_backward')
    return dx, dgamma, dbeta


def relu_clamp_backward(y, dy, dz):
    _check(load_library().nbasr_relu_clamp_backward(_dev(y, 'y'), _dev(dy, 'dy'), _dev(dz, 'dz'), y.numel(), _stream(y)), 'nbasr_relu_clamp_backward')
    return dz


def zero_stuff(dz, up, frames, frames_up, stride, shift):
    b, c, ld = dz.shape
    _check(load_library().nbasr_zero_stuff(_dev(dz, 'dz'), _dev(up, 'up'), b * c, frames, ld, frames_up, up.shape[2], stride, shift, _stream(dz)),
           'nbasr_zero_stuff')


def dense_conv1d_linear(x, frames, weight, bias, y, lpad):
    b, c_in, ld_in = x.shape
    c_out, _, kernel = weight.shape
    _check(load_library().nbasr_dense_conv1d_linear(_dev(x, 'x'), _dev(weight, 'weight'), _dev(bias, 'bias'), _dev(y, 'y'), b, c_in, frames, ld_in,
                                                    c_out, y.shape[2], kernel, lpad, _stream(x)), 'nbasr_dense_conv1d_linear')


def conv_cols(x, cols, frames_in, frames_out, t_pad, taps, stride, lpad):
    b, c_in, ld_in = x.shape
    _check(load_library().nbasr_conv_cols(_dev(x, 'x'), _dev(cols, 'cols'), b, c_in, frames_in, ld_in, frames_out, t_pad, taps, stride, lpad,
                                          cols.shape[-1], _stream(x)), 'nbasr_conv_cols')


def rows_of_channels(dz, rows, frames, t_pad):
    b, c, ld = dz.shape
    _check(load_library().nbasr_rows_of_channels(_dev(dz, 'dz'), _dev(rows, 'rows'), b, c, frames, ld, t_pad, _stream(dz)), 'nbasr_rows_of_channels')


def conv_fold(cols, dx, frames_in, frames_out, taps, stride, lpad):
    b, c_in, ld_in = dx.shape
    _check(load_library().nbasr_conv_fold(_dev(cols, 'cols'), _dev(dx, 'dx'), b, c_in, frames_in, ld_in, frames_out, taps, stride, lpad, _stream(dx)),
           'nbasr_conv_fold')


def lstm_gate_scan(pre, cells, batch):
    """Overwrites pre (4H, T, ldb) with the gate activations; cells (H, T, ldb) <- c_t."""
    hidden, frames, ldb = cells.shape
    _check(load_library().nbasr_lstm_gate_scan(_dev(pre, 'pre'), _dev(cells, 'cells'), hidden, frames, batch, ldb, _stream(pre)), 'nbasr_lstm_gate_scan')


def lstm_backward_step(dh_out, w_hh_t, dc, acts, cells, dpre, batch, t):
    hidden, frames, ldb = cells.shape
    _check(load_library().nbasr_lstm_backward_step(_dev(dh_out, 'dho'), _dev(w_hh_t, 'w_hh_t'), _dev(dc, 'dc'), _dev(acts, 'acts'), _dev(cells, 'cells'),
                                                   _dev(dpre, 'dpre'), hidden, frames, batch, ldb, t, _stream(dh_out)), 'nbasr_lstm_backward_step')
