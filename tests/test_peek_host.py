"""peek on the host: the planner's uncommitted steps leave it as it was and give the plans of a flush, their windows fit the session's
buffers, the three nbasr_ctc_beam_stream_*peek* entry points are declared, bound and exported and refuse bad arguments before any HIP
call, and the front-end's peek count is the flush's."""
import copy

import pytest

import cases
from nb_asr_amd import frontend, hip, streaming
from nbasr_header import declarations

NAMES = ('nbasr_ctc_beam_stream_peek_workspace_bytes', 'nbasr_ctc_beam_stream_peek', 'nbasr_ctc_beam_stream_timed_peek')
FIELDS = ('a', 'b', 'c', 'd', 'hist_off', 'n_hist', 'n_new', 'compute')
STATE = ('have', 'done', 'start', 'next_start', 'finished')
CHUNKINGS = ([1] * 40, [7] * 30, [64] * 12, [160, 0, 333, 5])


def plan_fields(plans):
    return [None if p is None else tuple(getattr(p, f) for f in FIELDS) for p in plans]


def planner_state(p):
    return copy.deepcopy(tuple(getattr(p, f) for f in STATE))


def steps_of(n, max_chunk):
    """A push of n frames as the session cuts it: steps of at most max_chunk frames, one empty step for an empty push."""
    return [min(max_chunk, n - off) for off in range(0, max(n, 1), max_chunk)]


@pytest.mark.parametrize('sizes', CHUNKINGS, ids=lambda s: f'{len(s)}x{s[0]}')
@pytest.mark.parametrize('use_rnn', [True, False])
@pytest.mark.parametrize('arch', ['A', 'D', 'M'])
def test_planner_peek_is_a_flush_that_did_not_happen(arch, use_rnn, sizes):
    specs = streaming.stage_specs(cases.ARCHS[arch], use_rnn)
    peeked, plain = streaming.StreamPlanner(specs), streaming.StreamPlanner(specs)
    max_chunk = 160
    caps = peeked.capacities(max_chunk)
    for n in sizes:
        for k in steps_of(n, max_chunk):
            assert plan_fields(peeked.step(k)) == plan_fields(plain.step(k))       # a peeked planner goes on like one never peeked
            before = planner_state(peeked)
            want = copy.deepcopy(peeked).step(0, final=True)
            got = peeked.peek()
            assert plan_fields(got) == plan_fields(want)
            assert planner_state(peeked) == before
            assert all(p is None or p.b - p.a <= cap for p, cap in zip(got, caps))
            # the chain of an audio session's flush: the front-end's end frames as a push, then the final step
            for m in (1, 2):
                twin = copy.deepcopy(peeked)
                want = [twin.step(m), twin.step(0, final=True)]
                throw_away = peeked.copy()
                got = [throw_away.step(m), throw_away.step(0, final=True)]
                assert [plan_fields(g) for g in got] == [plan_fields(w) for w in want]
                assert planner_state(peeked) == before
                assert all(p is None or p.b - p.a <= cap for g in got for p, cap in zip(g, caps))
                assert plan_fields(peeked.peek(m)) == plan_fields(copy.deepcopy(peeked).step(m, final=True))
                assert planner_state(peeked) == before
    assert plan_fields(peeked.step(0, final=True)) == plan_fields(plain.step(0, final=True))
    with pytest.raises(ValueError, match='reset'):
        peeked.peek()


@pytest.mark.parametrize('use_rnn', [True, False])
@pytest.mark.parametrize('arch,most', [('A', 127), ('D', 127), ('M', 45)])
def test_max_provisional_frames_is_the_brute_force_maximum(arch, use_rnn, most):
    """What sizes a session's beam peek workspace: the most frames a peek returns over the first lookahead + 600 single-frame steps, each
    peek counted on a throw-away planner -- the front-end's two end frames as a push, then the final step -- and without the end frames."""
    planner = streaming.StreamPlanner(streaming.stage_specs(cases.ARCHS[arch], use_rnn))
    before = planner_state(planner)
    got = planner.max_provisional_frames()
    assert planner_state(planner) == before
    with_end_frames = without = 0
    for _ in range(planner.lookahead + 600):
        planner.step(1)
        for end_frames in (2, 0):
            twin = planner.copy()
            twin.step(end_frames)
            twin.step(0, final=True)
            frames = twin.done[-1] - planner.done[-1]
            assert frames == hip.output_frames(planner.have[0] + end_frames) - planner.done[-1]
            if end_frames:
                with_end_frames = max(with_end_frames, frames)
            else:
                without = max(without, frames)
    assert got == with_end_frames == without == most


@pytest.mark.parametrize('name', NAMES)
def test_peek_symbols_are_declared_bound_and_exported(name):
    """That the binding's types are the header's is test_abi.py's check of every symbol."""
    ret, args = declarations()[name]
    lib = hip.load_library()
    assert getattr(lib, name).argtypes == hip.SIGNATURES[name][1]
    assert lib.nbasr_version() == 6
    if ret == 'int':
        state = args[2]
        assert state == 'const void* state', state                      # the state is only read


def test_peek_workspace_size():
    size = hip.load_library().nbasr_ctc_beam_stream_peek_workspace_bytes
    assert size(2, 10, 49, 33, 100) == 0 and size(2, 10, 65, 12, 100) == 0
    assert size(0, 10, 49, 12, 100) == 0 and size(2, 10, 49, 12, 0) == 0 and size(2, -1, 49, 12, 100) == 0
    for b, c, w in ((1, 49, 12), (3, 3, 1), (5, 64, 32)):
        last = 0
        for frames in (0, 1, 2, 33, 170):
            assert size(b, frames, c, w, 100) >= last > -1
            last = size(b, frames, c, w, 100)
            assert last % 8 == 0 and last > 0
            # room for the record's nodes and the chunk's in the wider (timed) node, and for the pruned chunk
            assert last >= b * (100 + w * frames + 1) * 16 + b * frames * c * 4
        last = 0
        for pool in (1, 2, 100, 1921, 50000):
            assert size(b, 33, c, w, pool) >= last
            last = size(b, 33, c, w, pool)
            assert last % 8 == 0


def _err(lib):
    return lib.nbasr_last_error()


@pytest.mark.parametrize('timed', [False, True])
def test_peek_refuses_bad_arguments_on_the_host(timed):
    lib = hip.load_library()
    p = 16                                            # a non-NULL, 8-byte aligned stand-in: every case is refused before a launch
    #      log_probs, lengths, state, ws, beams, scores, [timesteps,] beam_lens, ld, batch, frames, classes, width, blank, top_n, pool
    ok = [p, None, p, p, p, p] + ([p] if timed else []) + [p, 8, 2, 5, 49, 12, 0, 40, 100]
    at = {'log_probs': 0, 'state': 2, 'ws': 3, 'beams': 4, 'scores': 5}
    tail = {'lens': 0, 'ld': 1, 'batch': 2, 'frames': 3, 'classes': 4, 'width': 5, 'blank': 6, 'top_n': 7, 'pool': 8}
    at.update({k: v + (7 if timed else 6) for k, v in tail.items()})
    if timed:
        at['timesteps'] = 6
    fn = lib.nbasr_ctc_beam_stream_timed_peek if timed else lib.nbasr_ctc_beam_stream_peek

    def peek(**kw):
        a = list(ok)
        for k, v in kw.items():
            a[at[k]] = v
        return fn(*a, None)
    for null in ('state', 'ws', 'beams', 'scores', 'lens', 'log_probs') + (('timesteps',) if timed else ()):
        assert peek(**{null: None}) == -3 and b'NULL pointer' in _err(lib), null
    assert peek(width=33) == -1 and b'beam_width=33' in _err(lib)
    assert peek(width=0) == -1
    assert peek(classes=65) == -1 and b'classes=65' in _err(lib)
    assert peek(blank=49) == -1 and b'blank=49' in _err(lib)
    assert peek(pool=0) == -1 and b'pool_nodes=0' in _err(lib)
    assert peek(frames=-1) == -1 and peek(ld=-1) == -1 and peek(top_n=0) == -1
    assert peek(state=20) == -2 and b'8-byte aligned' in _err(lib)
    assert peek(ws=20) == -2
    assert peek(batch=0, state=None) == 0                               # nothing to do for an empty batch
    assert peek(frames=0, log_probs=None, state=None) == -3             # frames == 0 is legal, and is checked like any call


@pytest.mark.parametrize('samples', [0, 1, 200, 201, 360, 361, 16000])
def test_frontend_peek_count_is_the_flush_count(samples):
    if samples <= 200:
        assert frontend.frames_peek(samples) == 0
        with pytest.raises(ValueError):
            frontend.frames_total(samples)
    else:
        assert frontend.frames_peek(samples) == frontend.frames_total(samples) - frontend.frames_final(samples) in (1, 2)
