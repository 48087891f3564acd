"""The segmenter without a GPU: the definition (segment_model.py) on the hand-written cases, against a reading of it that searches for runs
instead of counting them, its invariants and invariances, ``SegmentRules`` validation and ``from_seconds``, the C entry points'
declarations, sizes and refusals, and the session's signature."""
import ctypes
import inspect
import itertools

import numpy as np
import pytest
import torch

from nb_asr_amd import ctc, hip, model as model_module, streaming
from nbasr_header import declarations
import segment_model as sm

S2 = (1,)                        # two classes: 0 = non-speech, 1 = speech


def mask_of(bits):
    return np.array([[int(ch) for ch in bits]], dtype=np.uint8).reshape(1, len(bits))


def run(bits, counts, capacity):
    """One row of decisions '0110...' through the automaton -> (head words as a dict, the ring as a list of tuples)."""
    state = sm.scan(mask_of(bits), None, None, *counts, capacity)
    assert not state[0, 5:8].any() and not sm.ring(state)[0, :, 3].any()
    return dict(zip(sm.FIELDS, (int(v) for v in state[0, :5]))), [tuple(int(v) for v in e[:3]) for e in sm.ring(state)[0]]


# ---- the model ---------------------------------------------------------------------------------------------------------------------
def test_hand_written_cases():
    assert sm.fresh(2, 1).tolist() == [[0, 0, 0, -1, 0, 0, 0, 0, -1, -1, -1, 0]] * 2 and sm.state_words(16) == 72
    head, ring = run('0011101100011110', (2, 2, 0), 4)
    # a pause of one frame (5) stays inside; the two silent frames 8, 9 close the segment at the first of them
    assert ring == [(2, 8, 0), (-1, -1, -1), (-1, -1, -1), (-1, -1, -1)]
    assert head == dict(frames=16, speech_run=0, silence_run=1, open_start=11, count=1)
    head, ring = run('1' * 10, (2, 2, 4), 4)
    # forced closes every four frames; after each the next segment needs two new speech frames and starts at the first of them
    assert ring[:2] == [(0, 4, 1), (4, 8, 1)] and head == dict(frames=10, speech_run=2, silence_run=0, open_start=8, count=2)
    head, ring = run('1010101010', (1, 1, 0), 2)
    # five segments of one frame through a ring of two: segment k lies in entry k % 2
    assert head['count'] == 5 and ring == [(8, 9, 0), (6, 7, 0)] and head['open_start'] == -1
    assert sm.spans(sm.scan(mask_of('1010101010'), None, None, 1, 1, 0, 2)) == [[(6, 7, 0), (8, 9, 0)]]
    assert sm.spans(sm.scan(mask_of('0011101100011110'), None, None, 2, 2, 0, 4), include_open=True) == [[(2, 8, 0), (11, 16, -1)]]
    assert run('', (1, 1, 0), 1) == (dict(frames=0, speech_run=0, silence_run=0, open_start=-1, count=0), [(-1, -1, -1)])


def by_search(bits, min_speech, min_silence, max_frames):
    """The definition read another way, as a search for runs in the whole string: from position p on, a segment starts at the first
    run of min_speech ones; it ends at the first run of min_silence zeros after that run, unless max_frames frames are complete
    before that run is; a forced close forgets the frames before it.  -> (closed segments, open_start, speech_run, silence_run)."""
    n, p, since, out = len(bits), 0, 0, []
    open_start = -1
    while True:
        start = bits.find('1' * min_speech, p)
        if start < 0:
            break
        quiet = bits.find('0' * min_silence, start + min_speech)
        closes_at = quiet + min_silence - 1 if quiet >= 0 else n                # the frame at which the silence rule holds
        forced_at = start + max_frames - 1 if max_frames else n
        if closes_at >= n and forced_at >= n:
            open_start = start
            break
        if closes_at <= forced_at:                                              # (at one frame, the silence rule comes first)
            out.append((start, quiet, 0))
            p = quiet + min_silence
        else:
            out.append((start, forced_at + 1, 1))
            p = since = forced_at + 1
    tail = bits[since:]
    return out, open_start, len(tail) - len(tail.rstrip('1')), len(tail) - len(tail.rstrip('0'))


@pytest.mark.parametrize('counts', [(1, 1, 0), (2, 2, 0), (2, 1, 3), (1, 3, 2), (3, 2, 5), (2, 2, 4)])
def test_the_model_equals_a_search_for_runs_on_every_mask_up_to_12_frames(counts):
    for n in range(13):
        for bits in map(''.join, itertools.product('01', repeat=n)):
            state = sm.scan(mask_of(bits), None, None, *counts, 16)
            closed, open_start, speech_run, silence_run = by_search(bits, *counts)
            assert sm.spans(state) == [closed], (bits, counts)
            assert state[0, :5].tolist() == [n, speech_run, silence_run, open_start, len(closed)], (bits, counts)


def random_case(seed, classes=9):
    rng = np.random.default_rng(seed)
    n, batch = int(rng.integers(1, 150)), int(rng.integers(1, 4))
    x = rng.standard_normal((batch, n, classes)).astype(np.float32)
    runs = np.repeat(rng.random((batch, n // 4 + 1)) < 0.5, 4, axis=1)[:, :n]   # speech and silence come in stretches
    x[runs ^ (rng.random((batch, n)) < 0.15), 0] += 3.0                         # class 0 (non-speech) wins there
    speech = tuple(sorted(rng.choice(np.arange(1, classes), size=int(rng.integers(1, classes - 1)), replace=False).tolist()))
    min_speech = int(rng.integers(1, 6))
    rules = (min_speech, int(rng.integers(1, 8)), int(rng.choice([0, min_speech + int(rng.integers(1, 20))])), int(rng.integers(1, 6)))
    lengths = rng.integers(0, n + 1, size=batch)
    return x, lengths, rules, speech


@pytest.mark.parametrize('seed', range(30))
def test_any_chunking_equals_the_whole_and_the_invariants_hold(seed):
    x, lengths, rules, speech = random_case(seed)
    whole, mask = sm.step(x, lengths, None, rules, speech, 0.0)
    rng = np.random.default_rng(seed + 1000)
    state, at, masks = None, 0, []
    n = x.shape[1]
    while at < n:
        k = min(int(rng.integers(0, 70)), n - at)
        state, m = sm.step(x[:, at:at + k], np.clip(lengths - at, 0, k), state, rules, speech, 0.0)
        masks.append(m)
        at += k
    assert np.array_equal(state, whole) and np.array_equal(np.concatenate(masks, 1), mask)
    # the invariants, on a ring that holds every segment
    min_speech, min_silence, max_frames, _ = rules
    full = sm.scan(mask, lengths, None, min_speech, min_silence, max_frames, 64)
    assert np.array_equal(full[:, :5], whole[:, :5]) and not whole[:, 5:8].any()
    assert sm.spans(whole) == [row[-rules[3]:] for row in sm.spans(full)]       # a smaller ring holds the last of them
    for b, row in enumerate(sm.spans(full, include_open=True)):
        frames, speech_run, silence_run, open_start, count = (int(v) for v in full[b, :5])
        assert frames == lengths[b] and min(speech_run, silence_run) == 0 and count == len([s for s in row if s[2] >= 0])
        last_end = 0
        for start, end, reason in row:
            assert last_end <= start < end <= frames                            # in the stream, ordered, disjoint
            assert end - start >= min_speech and mask[b, start:start + min_speech].all()
            if reason == 1:
                assert end - start == max_frames
            elif max_frames:
                assert end - start <= max_frames
            if reason == 0:
                assert not mask[b, end:end + min_silence].any() and mask[b, end - 1]
            last_end = end


@pytest.mark.parametrize('seed', range(10))
def test_a_shift_of_a_frame_changes_nothing(seed):
    """x + k per frame, every sum exact in float32: the same decisions at margin 0 and at a margin that is itself such a number."""
    x, lengths, rules, speech = random_case(seed)
    x = np.round(x * 64) / 64
    shift = np.random.default_rng(seed + 100).integers(-512, 512, size=x.shape[:2]).astype(np.float32)[..., None] / 8
    for margin in (0.0, 0.25):
        a = sm.step(x, lengths, None, rules, speech, margin)
        b = sm.step((x + shift).astype(np.float32), lengths, None, rules, speech, margin)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_nan_is_never_taken():
    x = np.array([[[1.0, 1.5], [np.nan, 5.0], [5.0, np.nan], [np.nan, np.nan], [-np.inf, 0.0], [2.0, 2.0]]], dtype=np.float32)
    state, mask = sm.step(x, None, None, (1, 1, 0, 4), S2, 0.0)
    assert mask.tolist() == [[1, 1, 0, 0, 1, 0]]
    assert sm.spans(state) == [[(0, 2, 0), (4, 5, 0)]]


# ---- the rules ---------------------------------------------------------------------------------------------------------------------
def test_defaults_and_from_seconds():
    rules = ctc.SegmentRules()
    assert rules.counts == (3, 13, 0, 16) and rules.speech_classes == ctc.default_speech_classes() and rules.classes == 49
    assert (rules.speech_lo, rules.speech_hi, rules.margin) == (ctc.EndpointRules().speech_lo, 0, 0.0)
    assert 'UNTUNED' in ctc.SegmentRules.__doc__
    assert ctc.SegmentRules.from_seconds().counts == rules.counts
    got = ctc.SegmentRules.from_seconds(0.05, 1.0, 20.0, capacity=4, margin=1.5)
    assert got.counts == (2, 25, 500, 4) and got.margin == 1.5
    with pytest.raises(ValueError, match='negative'):
        ctc.SegmentRules.from_seconds(min_silence=-0.1)
    with pytest.raises(ValueError, match='min_speech'):
        ctc.SegmentRules.from_seconds(min_speech=0.0)
    both = ctc.SegmentRules(1, 1, speech_classes=(1, 63, 64, 99), classes=100)
    assert both.speech_lo == (1 << 1) | (1 << 63) and both.speech_hi == 1 | (1 << 35)
    assert both._on(torch.device('cuda', 0)) is None                            # the counts travel by value: no device table


@pytest.mark.parametrize('kwargs,match', [
    (dict(classes=1, speech_classes=(0,)), 'classes'),
    (dict(classes=129, speech_classes=(0,)), 'classes'),
    (dict(classes=50), 'speech_classes must be given'),
    (dict(speech_classes=()), 'empty'),
    (dict(speech_classes=range(49)), 'every class'),
    (dict(speech_classes=(1, 49)), r'lie in \[0, 49\)'),
    (dict(speech_classes=(3, 3)), 'twice'),
    (dict(margin=-0.5), 'margin'),
    (dict(margin=float('nan')), 'margin'),
    (dict(min_speech=0), 'min_speech'),
    (dict(min_speech=-1), 'min_speech'),
    (dict(min_speech=1.5), 'min_speech'),
    (dict(min_speech=True), 'min_speech'),
    (dict(min_silence=0), 'min_silence'),
    (dict(min_silence=2 ** 31), 'min_silence'),
    (dict(min_speech=4, max_frames=4), 'max_frames'),
    (dict(min_speech=4, max_frames=1), 'max_frames'),
    (dict(max_frames=-1), 'max_frames'),
    (dict(capacity=0), 'capacity'),
    (dict(capacity=65), 'capacity'),
    (dict(device='cpu'), 'HIP device'),
])
def test_rules_validation(kwargs, match):
    with pytest.raises(ValueError, match=match):
        ctc.SegmentRules(**kwargs)


def test_the_edges_of_the_ranges_are_taken():
    assert ctc.SegmentRules(4, 1, 5, 64).counts == (4, 1, 5, 64) and ctc.SegmentRules(1, 1, 0, 1).counts == (1, 1, 0, 1)


def test_streams_functions_and_sessions_refuse_what_is_not_a_rule_set():
    with pytest.raises(ValueError, match='batch'):
        ctc.SegmentStream(0, ctc.SegmentRules())
    with pytest.raises(ValueError, match='SegmentRules'):
        ctc.SegmentStream(1, ctc.EndpointRules())
    with pytest.raises(ValueError, match='HIP device'):
        ctc.SegmentStream(1, ctc.SegmentRules(), device='cpu')
    with pytest.raises(ValueError, match='SegmentRules'):
        ctc.segment(torch.zeros(1, 2, 49), rules=(3, 13, 0))
    with pytest.raises(ValueError, match='HIP device'):
        ctc.segment(torch.zeros(1, 2, 49))
    with pytest.raises(ValueError, match='classes'):
        ctc.segment(torch.zeros(1, 2, 48))


def test_decode_spans_without_spans_needs_no_device():
    assert ctc.decode_spans(torch.zeros(3, 5, 49), [[], [], []]) == [[], [], []]
    for bad, match in ((dict(spans=[[]]), 'rows'), (dict(spans=[[(3, 2, 0)], [], []]), 'span'), (dict(spans=[[], [], []], pad=-1), 'pad')):
        with pytest.raises(ValueError, match=match):
            ctc.decode_spans(torch.zeros(3, 5, 49), **bad)
    params = inspect.signature(ctc.decode_spans).parameters
    assert list(params) == ['log_probs', 'spans', 'pad', 'beam_width', 'cutoff_top_n', 'lm', 'alpha', 'beta']
    assert [params[k].default for k in list(params)[2:]] == [0, 12, 40, None, 1.0, 0.0]
    assert all(params[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ('lm', 'alpha', 'beta'))


# ---- the C entry points ------------------------------------------------------------------------------------------------------------
def test_header_and_binding_entries():
    decl = declarations()
    assert decl['nbasr_ctc_segment_state_bytes'] == ('size_t', ['int batch', 'int capacity'])
    ret, params = decl['nbasr_ctc_segment_step']
    assert ret == 'int'
    assert [p.rsplit(' ', 1)[1].lstrip('*') for p in params] == ['x', 'lengths', 'state_in', 'state_out', 'min_speech', 'min_silence', 'max_frames',
                                                                'capacity', 'speech_lo', 'speech_hi', 'margin', 'mask_out', 'batch', 'frames',
                                                                'classes', 'stream']
    assert params[2].startswith('const int*') and params[3] == 'int* state_out'        # a peek's input state is const
    restype, argtypes = hip.SIGNATURES['nbasr_ctc_segment_step']
    assert restype is ctypes.c_int and len(argtypes) == 16
    assert all(t is ctypes.c_int for t in argtypes[4:8]) and argtypes[8] is argtypes[9] is ctypes.c_longlong and argtypes[10] is ctypes.c_float
    assert hip.SIGNATURES['nbasr_ctc_segment_state_bytes'] == (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int])
    lib = hip.load_library()
    assert lib.nbasr_ctc_segment_step.argtypes == argtypes and lib.nbasr_version() == 6     # additive: the ABI version stays
    assert 'segment.hip' in __import__('nb_asr_amd.build', fromlist=['SOURCES']).SOURCES


def test_state_bytes():
    lib = hip.load_library()
    for batch, capacity in ((1, 1), (5, 16), (64, 64), (3, 2)):
        assert lib.nbasr_ctc_segment_state_bytes(batch, capacity) == batch * (8 + 4 * capacity) * 4
        assert hip.ctc_segment_state_bytes(batch, capacity) == batch * hip.ctc_segment_state_words(capacity) * 4 == batch * sm.state_words(capacity) * 4
    assert [lib.nbasr_ctc_segment_state_bytes(b, s) for b, s in ((0, 4), (-3, 4), (2, 0), (2, 65), (2, -1))] == [0] * 5
    assert ctc._fresh_segment_state(2, 3).tolist() == sm.fresh(2, 3).tolist()


def test_refusals_without_a_device():
    """Every refusal of the step happens on the host, before a launch: dummy non-NULL addresses are never touched."""
    lib = hip.load_library()
    P = 4096                                                                            # stands for a device address
    good = dict(x=P, lengths=None, state_in=P, state_out=P, min_speech=3, min_silence=2, max_frames=0, capacity=4, lo=0b1010, hi=0, margin=0.0,
                mask=None, batch=2, frames=10, classes=49)

    def call(**change):
        a = dict(good, **change)
        rc = lib.nbasr_ctc_segment_step(a['x'], a['lengths'], a['state_in'], a['state_out'], a['min_speech'], a['min_silence'], a['max_frames'],
                                        a['capacity'], hip._signed64(a['lo']), hip._signed64(a['hi']), a['margin'], a['mask'], a['batch'],
                                        a['frames'], a['classes'], None)
        return rc, lib.nbasr_last_error()

    EINVAL, ENULL = -1, -3
    for change, code, text in [
        (dict(x=None), ENULL, b'NULL'),
        (dict(state_out=None), ENULL, b'NULL'),
        (dict(classes=1), EINVAL, b'classes=1 must lie in [2, 128]'),
        (dict(classes=129), EINVAL, b'classes'),
        (dict(lo=0), EINVAL, b'the speech set is empty'),
        (dict(lo=(1 << 49) - 1), EINVAL, b'the speech set is every class: no class is left for non-speech'),
        (dict(classes=128, lo=2 ** 64 - 1, hi=2 ** 64 - 1), EINVAL, b'every class'),
        (dict(classes=100, lo=2 ** 64 - 1, hi=(1 << 36) - 1), EINVAL, b'every class'),
        (dict(lo=1 << 49), EINVAL, b'the speech mask names classes at or above classes=49'),
        (dict(hi=1), EINVAL, b'at or above'),
        (dict(classes=100, lo=1, hi=1 << 36), EINVAL, b'at or above'),
        (dict(margin=-1.0), EINVAL, b'margin must be a number >= 0'),
        (dict(margin=float('nan')), EINVAL, b'margin'),
        (dict(batch=-1), EINVAL, b'negative sizes'),
        (dict(frames=-1), EINVAL, b'negative'),
        (dict(min_speech=0), EINVAL, b'min_speech'),
        (dict(min_silence=0), EINVAL, b'min_silence'),
        (dict(min_silence=-2), EINVAL, b'min_silence'),
        (dict(max_frames=3), EINVAL, b'max_frames'),
        (dict(max_frames=2), EINVAL, b'max_frames'),
        (dict(max_frames=-1), EINVAL, b'max_frames'),
        (dict(capacity=0), EINVAL, b'capacity'),
        (dict(capacity=65), EINVAL, b'capacity'),
    ]:
        rc, message = call(**change)
        assert rc == code and text in message and b'nbasr_ctc_segment_step' in message, (change, rc, message)
    # the wording of the shared refusals is the endpointer's, its own name apart
    rc, ours = call(lo=0)
    lib.nbasr_ctc_endpoint_step(P, None, P, P, P, 1, 0, 0, 0.0, None, 2, 10, 49, None)
    assert lib.nbasr_last_error().replace(b'endpoint', b'segment') == ours
    # nothing to do is not an error, and is decided on the host too: an empty batch; no frames with the state committed in place
    assert call(batch=0)[0] == 0
    assert call(frames=0, x=None)[0] == 0
    assert call(batch=0, x=None, frames=7)[0] == 0
    assert call(batch=0, max_frames=4, capacity=64)[0] == 0 and call(batch=0, capacity=1)[0] == 0          # the edges of the ranges are taken


# ---- the session's signature ---------------------------------------------------------------------------------------------------------
def test_session_signature():
    params = inspect.signature(streaming.StreamingSession.__init__).parameters
    names = list(params)
    assert params['segments'].kind is inspect.Parameter.KEYWORD_ONLY and params['segments'].default is None
    assert names.index('endpoint') < names.index('keywords') < names.index('segments') < names.index('lm') and names[-3:] == ['lm', 'alpha', 'beta']
    assert names[names.index('keywords') + 1] == 'segments' and names[names.index('segments') + 1] == 'lm'
    assert 'segments' not in inspect.signature(model_module.ASRModel.stream).parameters         # stream() keeps its parameter list
    assert isinstance(streaming.StreamingSession.segments, property) and callable(streaming.StreamingSession.peek_segments)
    assert 'provisional' in streaming.StreamingSession.peek_segments.__doc__.lower()
    assert 'open' in streaming.StreamingSession.segments.__doc__
