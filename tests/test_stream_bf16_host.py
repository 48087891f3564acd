"""bfloat16 streaming sessions, the part that needs no GPU: the C ABI of nbasr_stream_window_bf16 and every host-side refusal of it, the
``dtype`` keyword of ``StreamingSession``, and ``hip.round_up8``, the pitch of the session's bfloat16 windows."""
import ctypes
import inspect

import pytest
import torch

import cases
from nbasr_header import declarations
from nb_asr_amd import hip, streaming

EINVAL, EALIGN, ENULL = -1, -2, -3


def test_header_and_binding_entry():
    ret, params = declarations()['nbasr_stream_window_bf16']
    assert ret == 'int'
    assert [p.rsplit(' ', 1)[1].lstrip('*') for p in params] == ['hist', 'hist_ld', 'hist_off', 'n_hist', 'src', 'src_dtype', 'src_ld', 'src_off',
                                                                'n_new', 'dst', 'dst_ld', 'batch', 'channels', 'stream']
    assert params[0] == 'const void* hist' and params[4] == 'const void* src' and params[9] == 'void* dst'
    restype, argtypes = hip.SIGNATURES['nbasr_stream_window_bf16']
    assert restype is ctypes.c_int and len(argtypes) == len(params) == 14
    assert [i for i, t in enumerate(argtypes) if t is ctypes.c_void_p] == [0, 4, 9, 13]
    assert 'nbasr_stream_window_bf16' in hip._ENQUEUES and callable(hip.stream_window_bf16)
    assert hip.load_library().nbasr_version() == 6                                     # additive: the ABI version stays


def window(lib, hist=32, hist_ld=16, hist_off=0, n_hist=4, src=64, src_dtype=hip.BF16, src_ld=16, src_off=0, n_new=4, dst=96, dst_ld=8,
           batch=1, channels=2):
    """nbasr_stream_window_bf16 with made-up (never dereferenced) addresses: only calls the host checks refuse."""
    return lib.nbasr_stream_window_bf16(hist, hist_ld, hist_off, n_hist, src, src_dtype, src_ld, src_off, n_new, dst, dst_ld, batch, channels, None)


def test_every_refusal_answers_without_a_device():
    lib = hip.load_library()

    def err():
        return lib.nbasr_last_error()
    for bad in ({'batch': -1}, {'channels': 0}, {'n_hist': -1}, {'n_new': -1}, {'hist_off': -1}, {'src_off': -1}, {'dst_ld': -8}):
        assert window(lib, **bad) == EINVAL and b'bad sizes' in err(), bad
    assert window(lib, hist_off=13) == EINVAL and b'exceeds hist_ld' in err()
    assert window(lib, src_off=9, n_new=8, n_hist=0) == EINVAL and b'exceeds src_ld' in err()
    assert window(lib, n_hist=5) == EINVAL and b'do not fit' in err()
    for ld in (4, 12, 9, 15):
        assert window(lib, dst_ld=ld, n_hist=2, n_new=2) == EALIGN and b'multiple of 8' in err(), ld
    for code in (-1, 2, 7):
        assert window(lib, src_dtype=code) == EINVAL and b'src_dtype' in err(), code
    assert window(lib, hist=96) == EINVAL and b'different windows' in err()                       # hist == dst
    assert window(lib, dst=104) == EALIGN and b'16-byte' in err()
    assert window(lib, dst=None) == ENULL and window(lib, hist=None) == ENULL and window(lib, src=None) == ENULL and b'NULL' in err()
    assert window(lib, batch=1 << 20, channels=1 << 12) == EINVAL and b'rows' in err()
    # nothing to do: no launch, no pointer looked at
    assert window(lib, batch=0, dst=None) == 0 and window(lib, dst_ld=0, n_hist=0, n_new=0, dst=None) == 0


def test_session_signature():
    params = inspect.signature(streaming.StreamingSession.__init__).parameters
    names = list(params)
    assert params['dtype'].kind is inspect.Parameter.KEYWORD_ONLY and params['dtype'].default is None
    assert names[names.index('dtype') + 1] == 'input_rate' and params[names[names.index('dtype') - 1]].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD
    assert names[-3:] == ['lm', 'alpha', 'beta']
    # (ASRModel.stream keeps its parameter list -- tests/test_frontend_stream_host.py pins it --: like an LM or an input rate, the
    # bfloat16 session is an argument of the constructor, and stream()'s refusal of a bfloat16 model names it)
    assert 'bfloat16' in streaming.StreamingSession.__doc__ and 'dtype' in streaming.StreamingSession.__doc__


def test_round_up8_is_the_bf16_pitch_and_never_costs_more_bytes_than_fp32_rows():
    assert [hip.round_up8(n) for n in (0, 1, 7, 8, 9, 16, 17)] == [0, 8, 8, 8, 16, 16, 24]
    assert all(hip.round_up8(n) == hip.row_pitch(n, torch.bfloat16) for n in range(0, 70))
    for arch in (cases.ARCH_A, cases.ARCH_D, cases.ARCH_M):
        for use_rnn in (True, False):
            planner = streaming.StreamPlanner(streaming.stage_specs(arch, use_rnn))
            for max_chunk in (1, 40, 160):
                for cap in planner.capacities(max_chunk):
                    assert hip.round_up8(cap) * 2 <= hip.round_up4(cap) * 4, (arch, max_chunk, cap)


def test_a_dtype_that_is_no_storage_type_is_refused_before_anything_else():
    import nb_asr_amd as nb
    model = nb.get_model(cases.ARCH_A, use_rnn=True, dropout_rate=0.0).eval()
    for bad in (torch.float16, torch.float64, 'bf16'):
        with pytest.raises(ValueError, match='dtype'):
            streaming.StreamingSession(model, 1, dtype=bad)
    with pytest.raises(ValueError, match='does not match'):                        # a float32 model asked to run as bfloat16
        streaming.StreamingSession(model, 1, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match='does not match'):
        streaming.StreamingSession(model.to(torch.bfloat16), 1, dtype=torch.float32)
    with pytest.raises(ValueError, match=r'float32.*dtype=torch\.bfloat16'):          # the default names the keyword
        model.stream(batch=1)
