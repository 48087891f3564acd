"""The launch sequence of the training path's host algorithms, pinned: every enqueueing C-ABI call of ONE ``backward.dense_conv1d_backward``
/ ``backward.lstm_backward``, in order, with its arguments, compared with a recording made while the two functions still lived in the
binding (tests/golden/backward_launch_sequences.json).  Equal gradients do not show a GEMM that changed its batch, its padded row count
or its pitch, or a launch that moved; this does.

Arguments are normalised so that the listing does not depend on the allocator: integers and floats stay, a device address (or a
stream handle) becomes ``'ptr'``, a null pointer ``None``.  The cases are the smallest shapes that reach every branch of the two
functions, each under NBASR_DENSE_MODE=auto (the fp16-split GEMMs) and =f32 (the exact-fp32 route).

    python tests/test_backward_launch_gpu.py --record        # rewrites the fixture from the code as it is
"""
import ctypes
import json
import os
import pathlib
import sys

import pytest
import torch

REPO = pathlib.Path(__file__).resolve().parent.parent
if str(REPO) not in sys.path:
    sys.path.insert(0, str(REPO))

from nb_asr_amd import backward, hip                    # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
FIXTURE = REPO / 'tests' / 'golden' / 'backward_launch_sequences.json'
MODES = ('auto', 'f32')

# name: (c_in, c_out, kernel, stride, b, t, keyword arguments)
DENSE_CASES = {
    'dense_c24_40_s1_b2_t5': (24, 40, 8, 1, 2, 5, {}),                              # weight-gradient rows padded (40 -> 48)
    'dense_c24_48_s2_b3_t5': (24, 48, 8, 2, 3, 5, {}),                              # no row padding; stride-2 fold
    'dense_c5_12_s2_b2_t7': (5, 12, 8, 2, 2, 7, {}),                                # c_in * 8 % 16 != 0: zero-stuff route even in auto
    'dense_c24_40_s1_b1_t1': (24, 40, 8, 1, 1, 1, {}),                              # single frame
    'dense_c24_40_s1_b2_t5_dw_only': (24, 40, 8, 1, 2, 5, {'need_dx': False}),
    'dense_c24_40_s1_b2_t5_dx_only': (24, 40, 8, 1, 2, 5, {'need_dw': False}),
    'linear_c24_24_b2_t5': (24, 24, 1, 1, 2, 5, {'activation': True}),              # the `linear` op
    'head_c24_52_b2_t5': (24, 52, 1, 1, 2, 5, {'activation': False}),               # the head's form
}
# name: (c, hidden, b, t)
LSTM_CASES = {
    'lstm_c16_h4_b5_t1': (16, 4, 5, 1),                                             # b % 4 != 0; a single frame
    'lstm_c24_h8_b2_t5': (24, 8, 2, 5),                                             # several frames
    'lstm_c10_h12_b3_t4': (10, 12, 3, 4),                                           # c + 1 and 4 * hidden both need padding
}
CASES = [(name, mode) for name in list(DENSE_CASES) + list(LSTM_CASES) for mode in MODES]


def _pitched(gen, b, c, t, scale):
    x = torch.zeros(b, c, hip.round_up4(t))
    x[:, :, :t] = torch.randn(b, c, t, generator=gen) * scale
    return x


def dense_inputs(name):
    """(x, weight, y, dy, frames_in, stride), keyword arguments: values from a seeded CPU generator, the same in every process."""
    c_in, c_out, kernel, stride, b, t, kwargs = DENSE_CASES[name]
    gen = torch.Generator().manual_seed(sum(name.encode()))
    t_out = (t + stride - 1) // stride
    x = _pitched(gen, b, c_in, t, 3.0)
    w = torch.randn(*((c_out, c_in, 8) if kernel == 8 else (c_out, c_in)), generator=gen) * (2.0 / (c_in * kernel)) ** 0.5
    y = _pitched(gen, b, c_out, t_out, 8.0).clamp(0.0, 20.0)
    dy = _pitched(gen, b, c_out, t_out, 1e-2)
    return tuple(v.to(DEV) for v in (x, w, y, dy)) + (t, stride), kwargs


def lstm_inputs(name):
    """(xp, frames, gates, h_out, w_ih, w_hh, dh_out)."""
    c, hidden, b, t = LSTM_CASES[name]
    gen = torch.Generator().manual_seed(sum(name.encode()))
    xp = _pitched(gen, b, c, t, 1.5)
    gates = torch.randn(t, b, 4 * hidden, generator=gen)
    h_out = torch.tanh(torch.randn(b, t, hidden, generator=gen))
    w_ih, w_hh = torch.randn(4 * hidden, c, generator=gen) * 0.2, torch.randn(4 * hidden, hidden, generator=gen) * 0.2
    dh_out = torch.randn(b, t, hidden, generator=gen)
    xp, gates, h_out, w_ih, w_hh, dh_out = (v.to(DEV) for v in (xp, gates, h_out, w_ih, w_hh, dh_out))
    return xp, t, gates, h_out, w_ih, w_hh, dh_out


def run(name):
    """The case's gradients: (dx, dw, db) or (dx, dw_ih, dw_hh, db)."""
    if name in DENSE_CASES:
        args, kwargs = dense_inputs(name)
        return backward.dense_conv1d_backward(*args, **kwargs)
    return backward.lstm_backward(*lstm_inputs(name))


def normalise(entries):
    """[entry-point name, [arguments]] per entry; pointer-typed arguments by the signature table, not by their magnitude."""
    out = []
    for fn, args in entries:
        argtypes = hip.SIGNATURES[fn.__name__][1]
        assert len(argtypes) == len(args)
        out.append([fn.__name__, [(None if not a else 'ptr') if ty is ctypes.c_void_p else a for ty, a in zip(argtypes, args)]])
    return out


def record(name):
    entries = []
    hip.start_tape(entries)
    try:
        run(name)
    finally:
        hip.stop_tape()
    torch.cuda.synchronize()
    return normalise(entries)


@pytest.fixture(scope='module')
def pinned():
    return json.loads(FIXTURE.read_text())


@pytest.mark.parametrize('name,mode', CASES)
def test_backward_launch_sequence_is_the_recorded_one(monkeypatch, pinned, name, mode):
    monkeypatch.setenv('NBASR_DENSE_MODE', mode)
    got, want = record(name), pinned[f'{name}-{mode}']
    for i, (g, w) in enumerate(zip(got, want)):
        if g != w:
            print(f'{name}-{mode}: entry {i} of {len(got)} (recorded: {len(want)}) differs -- recorded\n  {w}\nnow\n  {g}')
            break
    assert [g[0] for g in got] == [w[0] for w in want]
    assert got == want


def record_all():
    """{case-mode: listing}; NBASR_DENSE_MODE is restored afterwards."""
    before = os.environ.get('NBASR_DENSE_MODE')
    try:
        out = {}
        for name, mode in CASES:
            os.environ['NBASR_DENSE_MODE'] = mode
            out[f'{name}-{mode}'] = record(name)
        return out
    finally:
        if before is None:
            os.environ.pop('NBASR_DENSE_MODE', None)
        else:
            os.environ['NBASR_DENSE_MODE'] = before


def write_fixture(listings):
    FIXTURE.write_text('{\n' + ',\n'.join(f'{json.dumps(k)}: {json.dumps(v)}' for k, v in listings.items()) + '\n}\n')


if __name__ == '__main__':
    if sys.argv[1:] != ['--record']:
        raise SystemExit(__doc__)
    from nb_asr_amd import build
    build.build_library()
    write_fixture(record_all())
    print(f'wrote {len(CASES)} cases to {FIXTURE}')
