"""Incremental front-end, the part that needs no GPU: which frames of a waveform stream are final and which samples must be kept
(frontend.frames_final / frames_total / retain_from) against numpy's reflect framing and against the oracle, the C ABI of
nbasr_frontend_stream_step and its host-side refusals, and the session's refusals that touch no device."""
import ctypes
import inspect
import math
import pathlib
import re

import numpy as np
import pytest
import torch

import nb_asr_amd as nb
from nb_asr_amd import frontend, hip, streaming
from oracle import frontend_oracle as fo

HEADER = pathlib.Path(__file__).resolve().parent.parent / 'include' / 'nbasr.h'
HOP, WIN = 160, 400
LENGTHS = (201, 320, 400, 1600, 1759, 4800, 12345, 16000)


def keyed_wave(seed, samples):
    rng = np.random.default_rng(seed)
    t = np.arange(samples) / 16000.0
    tone = 0.3 * np.sin(2 * math.pi * (200.0 + 37.0 * seed) * t) + 0.2 * np.sin(2 * math.pi * 3100.0 * t)
    return torch.from_numpy((tone + 0.1 * rng.standard_normal(samples)).astype(np.float32))


def chunkings(length):
    ragged, pattern, i = [], (3, 0, 411, 160, 1, 1000, 17, 0, 96), 0
    while sum(ragged) < length:
        ragged.append(min(pattern[i % len(pattern)], length - sum(ragged)))
        i += 1
    out = {'7': [min(7, length - i) for i in range(0, length, 7)], '160': [min(160, length - i) for i in range(0, length, 160)],
           'ragged': ragged, 'whole': [length]}
    if length <= 1759:
        out['1'] = [1] * length
    return out


def reference_frames(w):
    padded = np.pad(w, WIN // 2, 'reflect')
    return np.stack([padded[t * HOP:t * HOP + WIN] for t in range(len(w) // HOP + 1)])


def gather(held, first, frame, length=None):
    """The 400 samples of ``frame`` from the retained samples ``held`` (absolute index of held[0]: ``first``), as the kernel indexes them."""
    i = frame * HOP + np.arange(WIN) - WIN // 2
    i = np.where(i < 0, -i, i)
    if length is not None:
        i = np.where(i >= length, 2 * (length - 1) - i, i)
    assert i.min() >= first and i.max() < first + len(held), (frame, i.min(), i.max(), first, len(held))
    return held[i - first]


@pytest.mark.parametrize('length', LENGTHS)
def test_streamed_frames_equal_reflect_framing(length):
    w = np.random.default_rng(length).standard_normal(length)                 # float64
    want = reference_frames(w)
    assert frontend.frames_total(length) == len(want)
    for name, sizes in chunkings(length).items():
        held, first, seen, emitted, got = w[:0], 0, 0, 0, []
        for n in sizes:
            held = np.concatenate([held, w[seen:seen + n]])
            seen += n
            final = frontend.frames_final(seen)
            assert final == (0 if seen <= 200 else (seen - 200) // 160 + 1) and final >= emitted
            got += [gather(held, first, t) for t in range(emitted, final)]
            emitted = final
            keep = frontend.retain_from(emitted)
            assert keep == max(0, 160 * emitted - 201) and first <= keep <= seen
            held, first = held[keep - first:], keep
            assert len(held) <= 400, (name, seen, len(held))
        total = frontend.frames_total(seen)
        assert 1 <= total - emitted <= 2, (name, total, emitted)
        got += [gather(held, first, t, length) for t in range(emitted, total)]
        assert np.array_equal(np.stack(got), want), name


def test_flush_needs_more_than_half_a_window():
    for samples in (0, 1, 200):
        assert frontend.frames_final(samples) == 0
        with pytest.raises(ValueError, match='more than 200 samples'):
            frontend.frames_total(samples)
    assert frontend.frames_final(201) == 1 and frontend.frames_total(201) == 2
    assert frontend.frames_final(359) == 1 and frontend.frames_final(360) == 2


@pytest.mark.parametrize('length', (201, 360, 1000, 1759, 4800))
def test_finality_rule_is_safe_and_tight_on_the_oracle(length):
    """A frame below frames_final(L) has the same oracle features whatever follows sample L; frame frames_final(L) does not."""
    total = 6400
    w = keyed_wave(31, total).double()
    final = frontend.frames_final(length)
    garbage = w.clone()
    garbage[length:] = torch.from_numpy(np.random.default_rng(5).uniform(-1.0, 1.0, total - length))
    full, _ = fo.features([w], dtype=torch.float64)
    variants = [fo.features([w[:n]], dtype=torch.float64)[0] for n in sorted({length, length + 1, length + 159, length + 160, length + 401})]
    variants.append(fo.features([garbage], dtype=torch.float64)[0])
    for t in range(max(0, final - 3), final):
        for v in variants:
            assert float((v[0, :, t] - full[0, :, t]).abs().max()) <= 1e-12, (length, t)
    moved = max(float((v[0, :, final] - full[0, :, final]).abs().max()) for v in variants)
    assert moved > 1e-6, (length, final, moved)


def test_abi_lists_the_stream_entry_points(built_library):
    text = re.sub(r'/\*.*?\*/', '', HEADER.read_text(), flags=re.S)
    lib = ctypes.CDLL(str(built_library))
    for name in ('nbasr_frontend_stream_state_bytes', 'nbasr_frontend_stream_step'):
        assert re.search(r'\b' + name + r'\s*\(', text), name
        assert name in hip.SIGNATURES and hasattr(lib, name)
    assert hip.load_library().nbasr_version() == 6
    assert hip.frontend_stream_state_bytes(3, 400) == 2 * 3 * 404 * 4
    assert hip.frontend_stream_state_bytes(0, 400) == 0 and hip.frontend_stream_state_bytes(1, 0) == 0


def step(lib, tail_in=16, tail_len=0, tail_first=0, wave=16, n_new=1600, ld_wave=None, tail_out=32, rel=0, dft=16, fbank=16, mean=16,
         inv=16, feats=16, ld_feats=12, col0=0, first_frame=0, n_frames=9, total=None, final=0, batch=1, win=400, hop=160, bins=201, mels=80):
    """nbasr_frontend_stream_step with made-up (never dereferenced) addresses: only calls the host checks refuse."""
    total = tail_first + tail_len + n_new if total is None else total
    return lib.nbasr_frontend_stream_step(tail_in, tail_len, tail_first, wave, n_new, n_new if ld_wave is None else ld_wave, tail_out, rel, dft,
                                          fbank, mean, inv, feats, ld_feats, col0, first_frame, n_frames, total, final, batch, win, hop, bins,
                                          mels, None)


def test_step_refuses_bad_arguments_without_a_gpu():
    lib = hip.load_library()
    err = lambda: lib.nbasr_last_error()
    assert step(lib, win=512) == -1 and b'unsupported geometry' in err()
    assert step(lib, mels=40) == -1 and b'unsupported geometry' in err()
    assert step(lib, n_new=-1) == -1 and b'bad sizes' in err()
    assert step(lib, tail_len=405) == -1 and b'bad sizes' in err()
    assert step(lib, total=1700) == -1 and b'total_len' in err()
    assert step(lib, n_new=150, n_frames=0, final=1, tail_out=None) == -1 and b'reflect padding needs more than 200 samples' in err()
    assert step(lib, tail_len=200, n_new=0, wave=None, n_frames=0, final=1) == -1 and b'reflect' in err()
    assert step(lib, n_frames=0, n_new=0, wave=None) == 0                                   # nothing arrives, nothing to do
    assert step(lib, batch=0) == 0
    assert step(lib, batch=65536) == -1 and b'65535' in err()
    assert step(lib, wave=None) == -3 and b'NULL' in err()
    assert step(lib, tail_in=None, tail_len=100) == -3 and b'NULL' in err()
    assert step(lib, feats=None) == -3 and b'NULL' in err()
    assert step(lib, dft=None) == -3
    assert step(lib, ld_feats=10) == -2 and b'multiple of 4' in err()
    assert step(lib, dft=20) == -2
    assert step(lib, col0=4) == -1 and b'do not fit' in err()
    assert step(lib, n_frames=10, ld_feats=12) == -1 and b'need samples' in err()             # frame 9 ends at sample 1640
    assert step(lib, n_new=200, n_frames=1, ld_feats=4) == -1 and b'need samples' in err()    # frame 0 needs sample 200
    assert step(lib, tail_first=1000, tail_len=100, n_new=500, first_frame=7, n_frames=2, ld_feats=4) == -1 and b'need samples' in err()
    assert step(lib, tail_out=36) == -2 and b'16-byte' in err()
    assert step(lib, tail_in=32, tail_out=32) == -1 and b'in turn' in err()
    assert step(lib, rel=1000) == -1 and b'retaining 600 samples' in err()
    assert step(lib, rel=1601) == -1


def test_stream_signature_and_deviceless_refusals():
    model = nb.get_model([[1, 0], [1, 0, 0], [1, 0, 0, 0]], use_rnn=True, dropout_rate=0.0).eval()
    sig = inspect.signature(type(model).stream)
    assert list(sig.parameters)[1:] == ['batch', 'max_chunk', 'beam_width', 'cutoff_top_n', 'frontend'] and sig.parameters['frontend'].default is None
    assert 'frontend' in inspect.signature(streaming.StreamingSession.__init__).parameters
    with pytest.raises(ValueError, match='LogMelFrontend'):
        model.stream(batch=1, frontend='log-mel')
    with pytest.raises(ValueError, match='HIP device'):                       # (unchanged: a CPU model has no session)
        model.stream(batch=1)
    bare = object.__new__(streaming.StreamingSession)                         # a session made without a front-end
    bare._frontend = None
    with pytest.raises(ValueError, match='front-end'):
        bare.push_audio(torch.zeros(1, 160))
    for name in ('push', 'push_tiled', 'flush', 'reset'):
        assert callable(getattr(frontend.FrontendStream, name))
    assert callable(frontend.LogMelFrontend.stream) and callable(hip.frontend_stream_step)
