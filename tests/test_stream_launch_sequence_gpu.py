"""The launch sequence of a streaming session, pinned: every enqueueing C-ABI call of pushes, peeks and the flush of one utterance, in
order, with its arguments, compared with a recording made before ``StreamingSession`` got its carried-state record -- the bfloat16
scenarios: before it got its stage engines -- (tests/golden/stream_launch_sequences.json, stream_launch_sequences_bf16.json).
Bit-identical logits do not show a window built in another buffer, a state copy that changed hands or a launch that moved; this
does.  The listing and its summary are tests/test_launch_sequence_gpu.py's.

A scenario builds its session on a model with keyed parameters, runs its script once as a warm-up (every lazily made buffer, decoder
and peek workspace exists after it), calls ``reset()`` and runs the same script again on the tape.

Arguments are normalised so that the listing depends neither on the caching allocator nor on attribute names: small integers, floats
and None stay; a device address inside a model parameter becomes ``param:<state_dict key>``; one inside a tensor the session owns
becomes ``own<i>+<byte offset>``, ``i`` numbering the owned allocations by first appearance in the recorded pass; everything else is
``other`` (chunks, returned logits, beam outputs, stream handles).  The owned tensors are found by walking the session object
(``vars()`` of the package's objects, lists, tuples, dicts), not by a list of attribute names.

    python tests/test_stream_launch_sequence_gpu.py --record        # rewrites the fixture from the code as it is
"""
import json
import pathlib
import sys

import pytest
import torch

REPO = pathlib.Path(__file__).resolve().parent.parent
if str(REPO) not in sys.path:
    sys.path.insert(0, str(REPO))

import cases                                            # noqa: E402
import nb_asr_amd as nb                                 # noqa: E402
from nb_asr_amd import ctc, frontend, hip, streaming    # noqa: E402
from nb_asr_amd.utils import keyed_uniform              # noqa: E402
from nb_asr_amd.weights import keyed_input              # noqa: E402
from test_frontend_stream_gpu import keyed_wave         # noqa: E402
from test_launch_sequence_gpu import summarise          # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
BF16 = torch.bfloat16
FIXTURE = REPO / 'tests' / 'golden' / 'stream_launch_sequences.json'
FIXTURE_BF16 = FIXTURE.with_name('stream_launch_sequences_bf16.json')      # the bfloat16 scenarios: a file of their own, the first stays as it was
WIDTH = 4                       # the decoders' initial pool (1 + 4 * 160 nodes) holds every step: a step needs usage + 4 n + 1 of them

_models = {}


def model_for(arch, use_rnn, dtype=torch.float32):
    """One model per (architecture, LSTM or not, storage type), with keyed parameters (float32 values, then the cast: ``Module.to``
    converts in place, so a bfloat16 model is one of its own)."""
    key = (json.dumps(arch), use_rnn, dtype)
    if key not in _models:
        m = nb.get_model(arch, use_rnn=use_rnn, dropout_rate=0.0)
        m.load_state_dict(cases.keyed_params({k: tuple(v.shape) for k, v in m.state_dict().items()}, f'stream-launch/{key[0]}/{use_rnn}'))
        _models[key] = m.to(DEV).to(dtype).eval()
    return _models[key]


def features(b, t, seed):
    return keyed_input(b, t, seed=seed).to(DEV)


def waves(b, samples, seed):
    return torch.stack([keyed_wave(seed + i, samples) for i in range(b)]).to(DEV)


def keyed_lm():
    targets = 1 + (keyed_uniform('stream-launch/targets', 5, (16, 20), 0.0, 1.0) * 48).astype('int64').clip(0, 47)
    return ctc.bigram_lm(torch.from_numpy(targets), torch.full((16,), 20))


def pushes(sess, x, sizes, decode, audio=False):
    """Feed ``x`` cut into ``sizes`` (along its last dimension), a peek after every push; then flush."""
    at = 0
    for n in sizes:
        piece = x[..., at:at + n]
        if audio:
            sess.push_audio(piece, decode=decode)
        else:
            sess.push(piece, decode=decode)
        at += n
        sess.peek(decode=decode)
    sess.flush(decode=decode)


def greedy():
    sess = model_for(cases.ARCH_M, True).stream(batch=2, max_chunk=64)
    x = features(2, 280, 1)

    def script():
        sess.peek(True)
        pushes(sess, x, (100, 150, 0, 30), True)
    return sess, script


def beam_lm():
    sess = streaming.StreamingSession(model_for(cases.ARCH_M, False), batch=1, max_chunk=160, beam_width=WIDTH, lm=keyed_lm())
    x = features(1, 237, 2)

    def script():
        pushes(sess, x, (200, 37), 'beam-timed')
        sess.reset()
        pushes(sess, x[:, :, :64], (64,), 'beam')
    return sess, script


def audio():
    sess = model_for(cases.ARCH_M, True).stream(batch=2, max_chunk=64, frontend=frontend.LogMelFrontend(device=DEV))
    wave = waves(2, 32801, 90)
    return sess, lambda: pushes(sess, wave, (32000, 801, 0), True, audio=True)


def audio_chunks_of_one():
    sess = model_for(cases.ARCH_M, True).stream(batch=1, max_chunk=1, frontend=frontend.LogMelFrontend(device=DEV))
    wave = waves(1, 6400, 95)
    return sess, lambda: pushes(sess, wave, (1600,) * 4, False, audio=True)


def node_by_node():
    sess = model_for(cases.ARCH_M, True).stream(batch=2, max_chunk=7)
    x = features(2, 250, 3)
    return sess, lambda: pushes(sess, x, (250,), False)


def fused_cells():
    """Not one of the five the session's restructuring was specified with: ARCH_M's ``linear`` node keeps every one of them on the
    node-by-node route, so this one pins the one-launch cell (and the head without the LSTM after a peek)."""
    sess = model_for(cases.ARCH_A, False).stream(batch=2, max_chunk=160)
    x = features(2, 300, 4)
    return sess, lambda: pushes(sess, x, (300,), False)


def session16(arch, use_rnn, batch, max_chunk, **kw):
    return streaming.StreamingSession(model_for(arch, use_rnn, BF16), batch, max_chunk, dtype=BF16, **kw)


def bf16_greedy():
    """The bfloat16 session's node-by-node cells with a ``linear`` node (its input LayerNorm applied in place by the stage before), the
    on-load LayerNorm into the LSTM's projection, the recurrence, the head behind it, the peek's record and the widening for the decoder."""
    sess = session16(cases.ARCH_M, True, 2, 64)
    x = features(2, 280, 1).to(BF16)
    return sess, lambda: pushes(sess, x, (100, 150, 0, 30), True)


def bf16_mfma_cells_no_rnn():
    """... its matrix-core cells with their on-load statistics, the last LayerNorm written as the float32 rows the head without the LSTM
    reads, and two steps' logits joined over the padded bfloat16 buffer."""
    sess = session16(cases.ARCH_A, False, 2, 160)
    x = features(2, 300, 4).to(BF16)
    return sess, lambda: pushes(sess, x, (300,), False)


def bf16_audio_chunks_of_one():
    """... the front-end's float32 frames rounded while the first window is built, the peek's third buffers and its scratch window
    seen as bfloat16."""
    sess = session16(cases.ARCH_M, True, 1, 1, frontend=frontend.LogMelFrontend(device=DEV))
    wave = waves(1, 6400, 95)
    return sess, lambda: pushes(sess, wave, (1600,) * 4, False, audio=True)


SCENARIOS = {'greedy': greedy, 'beam_timed_lm_then_beam': beam_lm, 'audio': audio, 'audio_max_chunk_1': audio_chunks_of_one,
             'node_by_node_cells': node_by_node, 'fused_cells': fused_cells, 'bf16_greedy': bf16_greedy,
             'bf16_mfma_cells_no_rnn': bf16_mfma_cells_no_rnn, 'bf16_audio_max_chunk_1': bf16_audio_chunks_of_one}


def walk(sess):
    """(device tensors, beam decoders) reachable from the session, the model's modules left out."""
    seen, tensors, decoders = set(), [], []

    def visit(o):
        if id(o) in seen:
            return
        seen.add(id(o))
        if isinstance(o, torch.Tensor):
            if o.is_cuda:
                tensors.append(o)
        elif isinstance(o, torch.nn.Module):
            return
        elif isinstance(o, dict):
            for v in o.values():
                visit(v)
        elif isinstance(o, (list, tuple)):
            for v in o:
                visit(v)
        elif type(o).__module__.startswith('nb_asr_amd'):
            if isinstance(o, ctc.BeamSearchStream):
                decoders.append(o)
            visit(getattr(o, '__dict__', {}))
            for slot in getattr(type(o), '__slots__', ()):
                visit(getattr(o, slot, None))
    visit(sess)
    return tensors, decoders


def normalise(sess, entries):
    """One line per entry: ``name(arg, ...)``."""
    params = {v.data_ptr(): k for k, v in sess.model.state_dict().items()}
    tensors, _ = walk(sess)
    owned = {}                                          # allocation base -> bytes
    for t in tensors:
        s = t.untyped_storage()
        if s.data_ptr() not in params:
            owned[s.data_ptr()] = s.nbytes()
    numbers = {}

    def where(a):
        if isinstance(a, float) or a is None:
            return repr(a)
        if not isinstance(a, int):
            return type(a).__name__
        if a < (1 << 32):
            return repr(a)
        if a in params:
            return f'param:{params[a]}'
        for base, size in owned.items():
            if base <= a < base + size:
                return f'own{numbers.setdefault(base, len(numbers))}+{a - base}'
        return 'other'

    return [f"{e[0].__name__}({', '.join(where(a) for a in e[1])})" for e in entries]


def record(name):
    sess, script = SCENARIOS[name]()
    with torch.no_grad():
        script()                                        # warm-up: decoders, peek buffers and workspaces are made
        sess.reset()
        entries = []
        hip.start_tape(entries)
        try:
            script()
        finally:
            hip.stop_tape()
    torch.cuda.synchronize()
    _, decoders = walk(sess)
    assert all(d.grown == 0 for d in decoders), [d.grown for d in decoders]
    assert len(decoders) == (2 if name == 'beam_timed_lm_then_beam' else 0)
    return normalise(sess, entries)


@pytest.fixture(scope='module')
def pinned():
    return {**json.loads(FIXTURE.read_text()), **json.loads(FIXTURE_BF16.read_text())}


@pytest.mark.parametrize('name', list(SCENARIOS))
def test_stream_launch_sequence_is_the_recorded_one(pinned, name):
    lines = record(name)
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
    for path, names in ((FIXTURE, [n for n in SCENARIOS if not n.startswith('bf16_')]), (FIXTURE_BF16, [n for n in SCENARIOS if n.startswith('bf16_')])):
        path.write_text('{\n' + ',\n'.join(f'{json.dumps(name)}: {json.dumps(summarise(record(name)))}' for name in names) + '\n}\n')
        print(f'wrote {len(names)} scenarios to {path}')
