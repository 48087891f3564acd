"""The launch sequence of a forward, pinned: every enqueueing C-ABI call and host step of ONE forward through the python walk
(NBASR_TAPE=0), in order, with its arguments, compared with a recording made before the walk was split into per-layer steps
(tests/golden/launch_sequences.json).  Bit-identical logits do not show a launch that moved, a workspace that changed hands or a
derived weight built in another order; this does.

Arguments are normalised so that the listing does not depend on where the caching allocator puts things: small integers, floats
and None stay; a device address becomes the thing it points into -- ``buf:<workspace>+<byte offset>``, ``packed:<tag>@<parameter>``
(a derived weight copy), ``param:<state_dict key>``, ``x`` (the caller's input) or ``other`` (the returned logits, a tap copy, a
stream handle); a pending LayerNorm's descriptor is expanded into its three addresses.

    python tests/test_launch_sequence_gpu.py --record        # rewrites the fixture from the code as it is
"""
import contextlib
import hashlib
import json
import os
import pathlib
import sys

import pytest
import torch

REPO = pathlib.Path(__file__).resolve().parent.parent
if str(REPO) not in sys.path:
    sys.path.insert(0, str(REPO))

import cases                                            # noqa: E402
import nb_asr_amd as nb                                 # noqa: E402
from nb_asr_amd import hip                              # noqa: E402
from nb_asr_amd.weights import keyed_input              # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
FIXTURE = REPO / 'tests' / 'golden' / 'launch_sequences.json'
F32, BF16 = torch.float32, torch.bfloat16

_ROWS = {row[0]: row for row in cases.MODEL_CASES + cases.BF16_CASES}
_ROWS['A_lively_b1_t1100'] = ('A_lively_b1_t1100', cases.ARCH_A, True, 'lively', 1, 1100)       # block-0 rows longer than a workgroup


def _case(row, dtype, route='plain', **env):
    name = '-'.join([row, 'bf16' if dtype is BF16 else 'f32', route] + [f'{k}={v}' for k, v in env.items()])
    return name, (row, dtype, route, env)


CASES = dict(
    [_case(row, F32) for row in ('A_lively_b2_t67', 'D_xavier_b1_t200', 'M_lively_b2_t40_nornn', 'M_lively_b1_t90', 'A_lively_b1_t1100')]
    + [_case('D_xavier_b1_t200', F32, route) for route in ('taps', 'async', 'many')]
    + [_case('D_xavier_b1_t200', F32, **{k: v}) for k, v in (('NBASR_CELL_FUSION', '0'), ('NBASR_DENSE_MODE', 'f32'), ('NBASR_DENSE_MODE', 'bf16x3'),
                                                             ('NBASR_LINEAR_MODE', 'f32'), ('NBASR_CONV_STATS', '0'))]
    + [_case('M_lively_b1_t90', F32, NBASR_LINEAR_MODE='f32')]
    + [_case(row[0], BF16) for row in cases.BF16_CASES]
    + [_case('D_lively_b2_t200', BF16, route) for route in ('taps', 'async')]
    + [_case('D_lively_b2_t200', BF16, NBASR_CELL_FUSION=v) for v in ('valu', '0')])


@contextlib.contextmanager
def environment(env):
    env = dict(env, NBASR_TAPE='0')
    before = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in before.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


_models = {}


def model_for(row, dtype):
    """One model per (architecture, LSTM or not, storage type): the launch sequence does not depend on parameter VALUES."""
    _, arch, use_rnn, _, _, _ = _ROWS[row]
    key = (json.dumps(arch), use_rnn, dtype)
    if key not in _models:
        m = nb.get_model(arch, use_rnn=use_rnn, dropout_rate=0.0)
        m.load_state_dict(cases.keyed_params({k: tuple(v.shape) for k, v in m.state_dict().items()}, f'launch/{key[0]}/{use_rnn}'))
        _models[key] = m.to(DEV).to(dtype).eval()
    return _models[key]


def record(row, dtype, route, env):
    """(plan, model, x, entries) of the SECOND forward of this case."""
    _, _, _, _, b, t = _ROWS[row]
    m = model_for(row, dtype)
    x = keyed_input(b, t, seed=0).to(DEV).to(dtype)
    call = {'plain': lambda: m(x), 'taps': lambda: m.forward_with_taps(x), 'async': lambda: m.forward_async(x).result(),
            'many': lambda: m.forward_many([x, x], in_flight=1, tail_group=2)}[route]
    with environment(env), torch.no_grad():
        m._plans.clear()
        try:
            call()                                      # warm-up: workspaces grow, derived weights are built
            (plan,) = m._plans.values()
            entries = []
            plan._recording = entries
            hip.start_tape(entries)
            try:
                call()
            finally:
                hip.stop_tape()
                plan._recording = None
            torch.cuda.synchronize()
            return normalise(plan, m, x, entries)
        finally:
            m._plans.clear()


def normalise(plan, model, x, entries):
    """One line per entry: ``name(arg, ...)`` for a library call, ``host`` for a host step."""
    params = {v.data_ptr(): k for k, v in model.state_dict().items()}
    keys = {id(p): k for k, p in model.named_parameters()}
    packed = [(built.data_ptr(), built.numel() * built.element_size(), f'packed:{tag}@{keys.get(pid, "?")}')
              for (pid, tag), (_, _, built) in plan._packed.items() if isinstance(built, torch.Tensor)]
    bufs = [(t.data_ptr(), t.numel() * t.element_size(), name) for name, t in plan._bufs.items()]

    def where(a):
        if not isinstance(a, int) or isinstance(a, bool) or a < (1 << 32):
            return repr(a)
        if a == x.data_ptr():
            return 'x'
        for base, size, name in bufs:
            if base <= a < base + size:
                return f'buf:{name}+{a - base}'
        for base, size, label in packed:
            if base <= a < base + size:
                return label
        return f'param:{params[a]}' if a in params else 'other'

    def arg(a):
        ln = getattr(a, '_obj', None)                   # byref(DeferredLN)
        if ln is not None:
            return f'ln({where(ln.stats)}, {where(ln.gamma)}, {where(ln.beta)})'
        return where(a)

    return ['host' if e[0] is None else f"{e[0].__name__}({', '.join(arg(a) for a in e[1])})" for e in entries]


def summarise(lines):
    return {'names': [line.split('(')[0] for line in lines],
            'digests': [hashlib.sha256(line.encode()).hexdigest()[:8] for line in lines],
            'sha256': hashlib.sha256('\n'.join(lines).encode()).hexdigest()}


@pytest.fixture(scope='module')
def pinned():
    return json.loads(FIXTURE.read_text())


@pytest.mark.parametrize('name', list(CASES))
def test_launch_sequence_is_the_recorded_one(pinned, name):
    lines = record(*CASES[name])
    got, want = summarise(lines), pinned[name]
    if got != want:
        for i, line in enumerate(lines):
            if i >= len(want['names']) or (got['names'][i], got['digests'][i]) != (want['names'][i], want['digests'][i]):
                print(f'{name}: entry {i} of {len(lines)} (recorded: {len(want["names"])}) differs -- recorded '
                      f'{want["names"][i] if i < len(want["names"]) else "nothing"}, now\n  {line}')
                break
        else:
            print(f'{name}: {len(lines)} entries, recorded {len(want["names"])}: the sequence stops short')
    assert got['names'] == want['names']
    assert got['digests'] == want['digests'] and got['sha256'] == want['sha256']


if __name__ == '__main__':
    if sys.argv[1:] != ['--record']:
        raise SystemExit(__doc__)
    from nb_asr_amd import build
    build.build_library()
    FIXTURE.write_text('{\n' + ',\n'.join(f'{json.dumps(name)}: {json.dumps(summarise(record(*spec)))}' for name, spec in CASES.items()) + '\n}\n')
    print(f'wrote {len(CASES)} cases to {FIXTURE}')
