"""ctypes binding of libnbasr_hip.so (C ABI declared in include/nbasr.h).

PyTorch is used here only as plumbing: device memory (``tensor.data_ptr()``) and the current HIP stream.  Every wrapper validates device /
dtype / contiguity on the host, passes raw pointers and sizes, and raises ``HipError`` with the library's message on a non-zero return code.
A wrapper allocates at most its outputs and scratch; the host algorithms that string wrappers together are next door (walk.py: the forward;
backward.py: the dense and LSTM gradients).  There is NO fallback: a missing library or a tensor off the HIP device fails loudly (build
with ``python -m nb_asr_amd.build``).

This module is the core: the loaded library and the tape (``LIB_PATH``, ``_lib``, ``_tls``), the one table ``SIGNATURES`` and the helpers every wrapper
shares (``_call``, ``_scratch``, ``_opaque``, the pointer checks).  The wrappers live by kernel family in encoder, recurrent, audio, decode, detect and
train, which import from here only and are imported at this module's end.  A new entry point goes into include/nbasr.h and ONE family module: its
``(restype, argtypes)`` in the table that opens the module, its wrapper below.
"""
import ctypes
import os
import threading
import pathlib

import torch

LIB_PATH = pathlib.Path(__file__).resolve().parent.parent / 'lib' / 'libnbasr_hip.so'
ABI_VERSION = 6

_c_float_p = ctypes.c_void_p      # device pointers travel as opaque addresses
_c_int = ctypes.c_int
_c_stream = ctypes.c_void_p

class DeferredLN(ctypes.Structure):
    """struct nbasr_deferred_ln: per-frame statistics + affine parameters of a pending LayerNorm."""
    _fields_ = [('stats', ctypes.c_void_p), ('gamma', ctypes.c_void_p), ('beta', ctypes.c_void_p)]


_c_ln_p = ctypes.POINTER(DeferredLN)

# name -> (restype, argtypes) of every symbol declared in include/nbasr.h: the entries of the core here, every family module adds its own
SIGNATURES = {
    'nbasr_version': (_c_int, []),
    'nbasr_build_id': (ctypes.c_char_p, []),
    'nbasr_last_error': (ctypes.c_char_p, []),
    'nbasr_pad_amounts': (_c_int, [_c_int, _c_int, _c_int, ctypes.POINTER(_c_int), ctypes.POINTER(_c_int)]),
    'nbasr_output_frames': (_c_int, [_c_int]),
    'nbasr_stream_create': (_c_int, [ctypes.POINTER(ctypes.c_void_p)]),
}

# entry points that only answer on the host (never recorded on a launch tape); every other one enqueues work on a stream
_HOST_ONLY = frozenset({'nbasr_version', 'nbasr_build_id', 'nbasr_last_error', 'nbasr_pad_amounts', 'nbasr_output_frames', 'nbasr_stream_create',
                        'nbasr_grouped_cell_fits', 'nbasr_grouped_cell_mfma_fits'})

F32, BF16 = 0, 1                 # NBASR_F32 / NBASR_BF16


class HipError(RuntimeError):
    """``code``: the entry point's return value (a negative NBASR_E* argument error or a positive hipError_t), None for errors raised
    on the python side."""
    code = None


_lib = None
_tls = threading.local()


class _TapingLibrary:
    """Stand-in for the loaded library while a ``ForwardPlan`` records a launch tape (tape.LaunchTape): every entry point that takes a stream
    -- i.e. enqueues work -- is executed AND appended to ``entries`` as ``[function, [args]]``; host-only queries pass straight through."""

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
        raise HipError(f'{p} not found: the HIP extension has not been built (run `python -m nb_asr_amd.build`); there is no CPU fallback')
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


def _call(name, *args):
    """Call the entry point ``name`` of the library -- of the recording tape while one is active -- and raise on a non-zero code."""
    _check(getattr(load_library(), name)(*args), name)


def _scratch(nbytes, device, dtype=torch.uint8, least=8):
    """The one place a byte count of a ``*_bytes`` query becomes a tensor: ``dtype`` elements that cover ``nbytes`` bytes, rounded UP,
    and at least ``least`` bytes, so that ``data_ptr()`` is never null."""
    return torch.empty(-(-max(int(nbytes), least, 1) // dtype.itemsize), dtype=dtype, device=device)


def _opaque(t, nbytes, what, exact=False, dtype=torch.uint8, device=None):
    """The one check of an opaque image (packed weights, a workspace, a state): ``t`` is a contiguous tensor on a HIP device -- on
    ``device`` if given, of ``dtype`` unless that is None -- of at least, with ``exact`` of exactly, ``nbytes`` bytes.  Raises ``HipError``
    with the caller's words: ``what``, or ``(format, *values)`` where the check runs per launch and should format only when it fails."""
    have = t.numel() * t.element_size() if getattr(t, 'is_cuda', False) else -1
    if (have < nbytes or (exact and have != nbytes) or not t.is_contiguous() or (dtype is not None and t.dtype != dtype)
            or (device is not None and t.device != device)):
        raise HipError(what if isinstance(what, str) else what[0].format(*what[1:]))
    return t


def _stream(t):
    return torch.cuda.current_stream(t.device).cuda_stream


def _dev(t, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise HipError(f'{name} must be a tensor on a HIP device (got {getattr(t, "device", type(t))}); this package has no CPU path')
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
        raise HipError(f'{name} must be a tensor on a HIP device (got {getattr(t, "device", type(t))}); this package has no CPU path')
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


def _ptr(t):
    return None if t is None else t.data_ptr()


def _state(state, what='state'):
    if not isinstance(state, torch.Tensor) or not state.is_cuda or not state.is_contiguous():
        raise HipError(f'{what} must be a contiguous tensor on a HIP device')
    return state.data_ptr()


def _int_tensor(t, what, device, shape=None):
    if not t.is_cuda or t.device != device or t.dtype != torch.int32 or not t.is_contiguous():
        raise HipError(f'{what} must be a contiguous int32 tensor on {device}')
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise HipError(f'{what} must have shape {tuple(shape)}, got {tuple(t.shape)}')
    return t


def _lengths_ptr(lengths, batch):
    if lengths is None:
        return None
    if not lengths.is_cuda or lengths.dtype != torch.int32 or not lengths.is_contiguous() or lengths.numel() != batch:
        raise HipError('lengths must be a contiguous int32 device tensor with one entry per utterance')
    return lengths.data_ptr()


def _skips3(skips):
    return list(skips) + [None] * (3 - len(skips))


# host-only helpers (usable without a GPU)
def pad_amounts(kernel, dilation, stride):
    left, right = _c_int(), _c_int()
    _call('nbasr_pad_amounts', kernel, dilation, stride, ctypes.byref(left), ctypes.byref(right))
    return left.value, right.value


def output_frames(frames):
    return load_library().nbasr_output_frames(frames)


def round_up4(n):
    return (n + 3) & ~3


def round_up8(n):
    """The row pitch of bfloat16 rows: whole 16-byte chunks of 8 frames."""
    return (n + 7) & ~7


def dense_mode():
    """NBASR_DENSE_MODE as it is set NOW, validated; the one place that reads it.  Dense k = 8 convs, fp32-accurate in every mode: 'auto' (default)
    = 2-way fp16 split (3 MFMAs per product) wherever the input has just been written by the LayerNorm kernel (which also emits the per-utterance
    max|x| its range scaling needs), else the 3-way bf16 split (6 MFMAs, fp32's exponent range); 'bf16x3' = that everywhere; 'f32' = exact-fp32 MFMA."""
    mode = os.environ.get('NBASR_DENSE_MODE', 'auto')
    if mode not in ('auto', 'bf16x3', 'f32'):
        raise ValueError(f'NBASR_DENSE_MODE must be auto, bf16x3 or f32, got {mode!r}')
    return mode


# the families: each registers its signatures and defines its wrappers from the names bound above (``*`` skips their private names)
from .encoder import *      # noqa: E402,F401,F403
from .encoder import _scheme_code, _dense_packed, _check_packed      # noqa: E402,F401
from .recurrent import *    # noqa: E402,F401,F403
from .recurrent import _check_whh, _check_whh16, _check_pointwise, _check_pointwise_bf16      # noqa: E402,F401
from .audio import *        # noqa: E402,F401,F403
from .audio import _wave_rows, _tail_pair      # noqa: E402,F401
from .decode import *       # noqa: E402,F401,F403
from .decode import _BEAM_OPS, _BEAM_PICKERS, _beam_call, _fusion, _check_chunk, _check_stream_chunk, _beam_outputs, _ctc_args      # noqa: E402,F401
from .detect import *       # noqa: E402,F401,F403
from .detect import _signed64, _detector_step_args, _speech_mask_arg      # noqa: E402,F401
from .train import *        # noqa: E402,F401,F403    (below: the taped entry points, over the whole table)

_ENQUEUES = frozenset(name for name in SIGNATURES if name not in _HOST_ONLY and not name.endswith('_bytes') and '_bytes_' not in name)
