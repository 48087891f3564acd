"""The confidence estimator without a GPU: the definition (confidence_model.py) on the hand-written cases, against itertools.groupby on the
argmax, its invariants and invariances, the bound on q and a wrong formula that the comparison helper must catch, ``ConfidenceRules``
validation, the C entry points' declarations, sizes and refusals, and the session's signature."""
import ctypes
import inspect
import itertools

import numpy as np
import pytest
import torch

from nb_asr_amd import ctc, hip, model as model_module, streaming
from nbasr_header import declarations
import confidence_model as cm

NEG = -np.inf


# ---- the model ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('classes', [2, 3, 49, 128])
def test_hand_written_cases(classes):
    one_hot = np.full((1, classes, classes), NEG, dtype=np.float32)
    one_hot[0, np.arange(classes), np.arange(classes)] = 3.5                    # frame t: everything on class t (masked classes are legal)
    peaked = np.where(np.isinf(one_hot), np.float32(-90.0), one_hot)            # ... and without a mask: exp(-93.5) is nothing
    uniform = np.full((1, 4, classes), 0.75, dtype=np.float32)
    for measure in cm.MEASURES:
        for dtype in (np.float64, np.float32):
            for x in (one_hot, peaked):
                labels, q, bad = cm.frames_q(x, measure, dtype=dtype)
                assert labels.tolist() == [list(range(classes))] and (q == cm.ONE).all() and not bad.any(), (measure, dtype)
            labels, q, _ = cm.frames_q(uniform, measure, dtype=dtype)
            assert labels.tolist() == [[0] * 4]                                 # every value is the largest: the lowest index
            want = round(cm.ONE / classes) if measure == 'prob' else 0
            assert np.abs(q - want).max() <= (cm.tolerance(classes, 0.75, measure) if dtype == np.float32 else 1), (measure, dtype, q)
    assert cm.fresh(2).tolist() == [[0, -1, -1, cm.ONE, 0, 0, 0, cm.ONE, 0, 0, 0, 0, 0, 0, 0, 0]] * 2
    assert ctc._fresh_confidence_state(2).tolist() == cm.fresh(2).tolist() and ctc.CONFIDENCE_ONE == cm.ONE


def test_tokens_by_hand():
    """a a blank a b b | final: the same label after a blank is a new token; blanks belong to none; the end closes the last."""
    labels = np.array([[1, 1, 0, 1, 2, 2]])
    q = np.array([[10, 30, 999, 7, 5, 6]])
    state, table, counts = cm.scan(labels, q, None, None, 0, True)
    assert cm.tokens_of(table, counts) == [[(1, 0, 2, 10, 40), (1, 3, 4, 7, 7), (2, 4, 6, 5, 11)]]
    assert (table[0, 3:] == -1).all() and table.shape == (1, 7, 8) and not table[0, :3, 6:].any()
    assert dict(zip(cm.FIELDS, state[0].tolist())) == dict(frames=6, prev_label=-1, open_start=-1, open_min_q=cm.ONE, open_sum_lo=0, open_sum_hi=0,
                                                           tokens=3, utt_min_q=5, utt_sum_lo=58, utt_sum_hi=0, utt_frames=5, bad=0)
    state, table, counts = cm.scan(labels, q, None, None, 0, False)             # not final: the last token stays open, in the record
    assert cm.tokens_of(table, counts) == [[(1, 0, 2, 10, 40), (1, 3, 4, 7, 7)]]
    assert state[0, :7].tolist() == [6, 2, 4, 5, 11, 0, 2]
    # a 64-bit sum: 300 frames of q = 2^24 pass 2^32
    state, table, counts = cm.scan(np.ones((1, 300), dtype=int), np.full((1, 300), cm.ONE), None, None, 0, True)
    assert cm.tokens_of(table, counts) == [[(1, 0, 300, cm.ONE, 300 * cm.ONE)]] and table[0, 0, 4:6].tolist() == [(300 * cm.ONE) & 0xFFFFFFFF, 1]
    assert cm.join(state[0, 8], state[0, 9]) == 300 * cm.ONE
    # every frame a new label, a carried token and final: frames + 1 tokens, the most a step can close
    first = cm.scan(np.array([[5]]), np.array([[1]]), None, None, 0, False)[0]
    state, table, counts = cm.scan(np.array([[1, 2, 3, 4]]), np.array([[1, 2, 3, 4]]), None, first, 0, True)
    assert counts.tolist() == [5] and [t[0] for t in cm.tokens_of(table, counts)[0]] == [5, 1, 2, 3, 4]


def random_case(seed, classes=None, scale=None):
    rng = np.random.default_rng(seed)
    classes = int(rng.choice([2, 3, 9, 49])) if classes is None else classes
    n, batch = int(rng.integers(1, 150)), int(rng.integers(1, 4))
    scale = float(rng.choice([0.5, 2.0, 8.0])) if scale is None else scale
    x = np.clip(rng.standard_normal((batch, n, classes)) * scale, -100, 100).astype(np.float32)
    stretch = np.repeat(rng.integers(0, classes, size=(batch, n // 3 + 1)), 3, axis=1)[:, :n]   # labels come in stretches
    np.put_along_axis(x, stretch[..., None], np.take_along_axis(x, stretch[..., None], 2) + np.float32(2 * scale), 2)
    lengths = rng.integers(0, n + 1, size=batch)
    return x, lengths


@pytest.mark.parametrize('seed', range(20))
def test_tokens_equal_groupby_on_the_argmax_and_the_invariants_hold(seed):
    x, lengths = random_case(seed)
    measure = cm.MEASURES[seed % 3]
    state, table, counts, trace = cm.step(x, lengths, None, measure, final=True)
    labels = np.argmax(x, axis=-1)
    for b, row in enumerate(cm.tokens_of(table, counts)):
        runs, t = [], 0
        for label, group in itertools.groupby(labels[b, :lengths[b]].tolist()):
            k = len(list(group))
            runs.append((label, t, t + k))
            t += k
        assert [r[:3] for r in row] == [r for r in runs if r[0] != 0]
        assert (trace[b, :lengths[b]] >= 0).all() and (trace[b, :lengths[b]] <= cm.ONE).all() and (trace[b, lengths[b]:] == -1).all()
        for label, start, end, min_q, sum_q in row:
            frames = trace[b, start:end]
            assert min_q == frames.min() and sum_q == int(frames.astype(np.int64).sum())
            assert 0 <= min_q * (end - start) <= sum_q <= cm.ONE * (end - start)
        spoken = trace[b, :lengths[b]][labels[b, :lengths[b]] != 0]
        assert state[b, 0] == lengths[b] and state[b, 6] == len(row) and state[b, 10] == len(spoken) and state[b, 1:3].tolist() == [-1, -1]
        assert state[b, 7] == (spoken.min() if len(spoken) else cm.ONE) and cm.join(state[b, 8], state[b, 9]) == int(spoken.sum())
        assert not state[b, 11:].any()


@pytest.mark.parametrize('seed', range(20))
def test_any_chunking_equals_the_whole(seed):
    x, lengths = random_case(seed)
    measure = cm.MEASURES[seed % 3]
    whole = cm.step(x, lengths, None, measure, final=True)
    rng = np.random.default_rng(seed + 1000)
    for last_is_final in (True, False):                          # ... or a final step of no frames after the last chunk
        state, at, n, tokens, traces = None, 0, x.shape[1], [[] for _ in lengths], []
        while at < n:
            k = min(int(rng.integers(0, 70)), n - at)
            state, table, counts, trace = cm.step(x[:, at:at + k], np.clip(lengths - at, 0, k), state, measure, final=last_is_final and at + k == n)
            assert table.shape[1] == k + 1
            tokens = [a + b for a, b in zip(tokens, cm.tokens_of(table, counts))]
            traces.append(trace)
            at += k
        if not last_is_final:
            state, table, counts, _ = cm.step(x[:, :0], None, state, measure, final=True)
            assert table.shape[1] == 1 and counts.max() <= 1
            tokens = [a + b for a, b in zip(tokens, cm.tokens_of(table, counts))]
        assert np.array_equal(state, whole[0]) and tokens == cm.tokens_of(whole[1], whole[2])
        assert np.array_equal(np.concatenate(traces, 1), whole[3])


@pytest.mark.parametrize('seed', range(10))
def test_a_shift_of_a_frame_changes_nothing_in_float64(seed):
    x, lengths = random_case(seed, scale=2.0)
    x = np.round(x * 64) / 64                                    # x + shift is exact in float32
    shift = np.random.default_rng(seed + 100).integers(-512, 512, size=x.shape[:2]).astype(np.float32)[..., None] / 8
    for measure in cm.MEASURES:
        a, b = cm.step(x, lengths, None, measure, final=True), cm.step((x + shift).astype(np.float32), lengths, None, measure, final=True)
        assert all(np.array_equal(u, v) for u, v in zip(a, b)), measure


def test_a_path_gives_the_labels_and_a_bad_one_counts_as_blank():
    x, _ = random_case(3, classes=9)
    x = x[:1, :12]
    path = np.array([[0, 4, 4, 0, 4, 7, 7, 9, 7, -1, 2, 2]])
    state, table, counts, trace = cm.step(x, None, None, 'prob', final=True, path=path)
    assert [t[:3] for t in cm.tokens_of(table, counts)[0]] == [(4, 1, 3), (4, 4, 5), (7, 5, 7), (7, 8, 9), (2, 10, 12)] and state[0, 11] == 1
    lp = x[0].astype(np.float64) - np.log(np.exp(x[0].astype(np.float64)).sum(-1, keepdims=True))
    want = np.rint(np.exp(lp[np.arange(12), np.where((path[0] < 0) | (path[0] > 8), 0, path[0])]) * cm.ONE)
    assert np.abs(trace[0] - want).max() <= 1                                   # prob: the path label's probability (a bad label: the blank's)
    assert cm.step(x, None, None, 'prob', final=True, path=np.clip(path, 0, 8))[0][0, 11] == 0


def test_mean_and_min_are_the_stated_function_of_the_integers():
    rng = np.random.default_rng(5)
    for _ in range(200):
        frames = int(rng.integers(1, 5000))
        min_q = int(rng.integers(0, cm.ONE + 1))
        sum_q = int(rng.integers(min_q * frames, cm.ONE * frames + 1))
        state = torch.tensor([[frames, 0, -1, cm.ONE, 0, 0, 1, min_q, *cm.split(sum_q), frames, 0, 0, 0, 0, 0]], dtype=torch.int32)
        table = torch.tensor([[[3, 10, 10 + frames, min_q, *cm.split(sum_q), 0, 0], [-1] * 8]], dtype=torch.int32)
        r = ctc.ConfidenceResult(state, table, torch.tensor([1], dtype=torch.int32))
        assert int(r.sum_q[0, 0]) == sum_q and r.sum_q.dtype == torch.int64 and int(r.sum_q[0, 1]) == -1
        for got, want in ((r.mean[0, 0], cm.mean_of(sum_q, frames)), (r.min[0, 0], cm.min_of(min_q)),
                          (r.utterance_mean[0], cm.mean_of(sum_q, frames)), (r.utterance_min[0], cm.min_of(min_q))):
            assert got.dtype == torch.float32 and got.numpy().tobytes() == np.float32(want).tobytes()
        assert 0.0 <= float(r.min[0, 0]) <= float(r.mean[0, 0]) <= 1.0 and torch.isnan(r.mean[0, 1]) and torch.isnan(r.min[0, 1])
        assert r.tokens_list() == [[(3, 10, 10 + frames, float(cm.mean_of(sum_q, frames)), float(cm.min_of(min_q)))]]
    nothing = ctc.ConfidenceResult(torch.from_numpy(cm.fresh(1)), torch.full((1, 1, 8), -1, dtype=torch.int32), torch.zeros(1, dtype=torch.int32))
    assert torch.isnan(nothing.utterance_mean[0]) and float(nothing.utterance_min[0]) == 1.0 and nothing.tokens_list() == [[]]


# ---- the bound on q ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('classes', [2, 3, 49, 128])
@pytest.mark.parametrize('scale', [1.0, 20.0])
def test_the_float32_model_is_within_the_bound_and_the_bound_within_the_cap(classes, scale):
    x, lengths = random_case(classes + int(scale), classes, scale)
    for measure, alpha in (('prob', 1 / 3), ('entropy', 1 / 3), ('tsallis', 1 / 3), ('tsallis', 0.5)):
        assert cm.tolerance(classes, 100.0, measure, alpha) <= cm.CAP           # the whole range the tests keep to, |x| <= 100
        assert cm.tolerance(classes, 1.0, measure, alpha) < cm.tolerance(classes, 100.0, measure, alpha)       # it grows with |x|
        _, q32, _ = cm.frames_q(x, measure, alpha, dtype=np.float32)
        worst = cm.assert_q_close(q32, x, lengths, measure, alpha)
        print(f'C={classes} scale={scale} {measure} alpha={alpha:.3f}: float32 numpy model at most {worst} units from float64')


@pytest.mark.parametrize('measure', cm.MEASURES)
def test_a_wrong_log_base_does_not_pass_the_comparison(measure):
    """log2 in place of ln in step 2: the normaliser is wrong, and the helper that every q is compared with says so."""
    x, lengths = random_case(11, classes=49, scale=2.0)
    lengths = np.full_like(lengths, x.shape[1])
    labels = cm.greedy_labels(x)
    right = cm.quantise(cm.frame_confidence(x, labels, measure))
    assert cm.assert_q_close(right, x, lengths, measure) == 0
    wrong = cm.quantise(cm.frame_confidence(x, labels, measure, log=np.log2))
    with pytest.raises(AssertionError):
        cm.assert_q_close(wrong, x, lengths, measure)
    assert np.abs(wrong - right).min() > cm.CAP or np.median(np.abs(wrong - right)) > cm.CAP    # far beyond the cap, at the typical frame


# ---- the rules ---------------------------------------------------------------------------------------------------------------------
def test_defaults():
    rules = ctc.ConfidenceRules()
    assert (rules.measure, rules.alpha, rules.blank, rules.classes, rules.measure_index) == ('tsallis', 1 / 3, 0, 49, 2)
    assert list(inspect.signature(ctc.ConfidenceRules.__init__).parameters)[1:] == ['measure', 'alpha', 'blank', 'classes', 'device']
    assert 'UNTUNED' in ctc.ConfidenceRules.__doc__
    assert ctc.CONFIDENCE_MEASURES == cm.MEASURES == hip.CONFIDENCE_MEASURES
    assert rules._on(torch.device('cuda', 0)) is None                           # everything travels by value: no device table
    assert ctc.ConfidenceRules('prob', alpha=0.999, blank=127, classes=128).blank == 127 and ctc.ConfidenceRules('entropy', classes=2).classes == 2


@pytest.mark.parametrize('kwargs,match', [
    (dict(measure='margin'), 'measure'),
    (dict(measure=2), 'measure'),
    (dict(alpha=0.0), 'alpha'),
    (dict(alpha=1.0), 'alpha'),
    (dict(alpha=-0.5), 'alpha'),
    (dict(alpha=float('nan')), 'alpha'),
    (dict(alpha='1/3'), 'alpha'),
    (dict(alpha=True), 'alpha'),
    (dict(classes=1), 'classes'),
    (dict(classes=129), 'classes'),
    (dict(classes=48.5), 'classes'),
    (dict(blank=-1), 'blank'),
    (dict(blank=49), 'blank'),
    (dict(blank=2, classes=2), 'blank'),
    (dict(device='cpu'), 'HIP device'),
])
def test_rules_validation(kwargs, match):
    with pytest.raises(ValueError, match=match):
        ctc.ConfidenceRules(**kwargs)


def test_streams_functions_and_sessions_refuse_what_is_not_a_rule_set():
    with pytest.raises(ValueError, match='batch'):
        ctc.ConfidenceStream(0, ctc.ConfidenceRules())
    with pytest.raises(ValueError, match='ConfidenceRules'):
        ctc.ConfidenceStream(1, ctc.EndpointRules())
    with pytest.raises(ValueError, match='HIP device'):
        ctc.ConfidenceStream(1, ctc.ConfidenceRules(), device='cpu')
    with pytest.raises(ValueError, match='ConfidenceRules'):
        ctc.confidence(torch.zeros(1, 2, 49), rules='tsallis')
    with pytest.raises(ValueError, match='HIP device'):
        ctc.confidence(torch.zeros(1, 2, 49))
    with pytest.raises(ValueError, match='classes'):
        ctc.confidence(torch.zeros(1, 2, 48))
    assert list(inspect.signature(ctc.confidence).parameters) == ['x', 'output_len', 'rules', 'path', 'return_frames']
    assert list(inspect.signature(ctc.path_confidence).parameters) == ['log_probs', 'output_len', 'targets', 'targets_len', 'rules']
    assert list(inspect.signature(ctc.ConfidenceStream.push).parameters) == ['self', 'x', 'lengths', 'final']
    assert inspect.signature(ctc.ConfidenceStream.peek).parameters['final'].default is True
    assert issubclass(ctc.ConfidenceStream, ctc._LogitDetectorStream)


# ---- the C entry points ------------------------------------------------------------------------------------------------------------
def test_header_and_binding_entries(built_library):
    decl = declarations()
    assert decl['nbasr_ctc_confidence_state_bytes'] == ('size_t', ['int batch'])
    ret, params = decl['nbasr_ctc_confidence_step']
    assert ret == 'int'
    assert [p.rsplit(' ', 1)[1].lstrip('*') for p in params] == ['x', 'lengths', 'path', 'state_in', 'state_out', 'measure', 'alpha', 'blank', 'final',
                                                                'tokens_out', 'token_counts', 'frame_q', 'batch', 'frames', 'classes', 'stream']
    assert params[3].startswith('const int*') and params[4] == 'int* state_out'        # a peek's input state is const
    restype, argtypes = hip.SIGNATURES['nbasr_ctc_confidence_step']
    assert restype is ctypes.c_int and len(argtypes) == 16
    assert [argtypes[i] for i in (5, 6, 7, 8)] == [ctypes.c_int, ctypes.c_float, ctypes.c_int, ctypes.c_int]
    assert all(t is ctypes.c_void_p for t in argtypes[:5] + argtypes[9:12] + argtypes[15:])
    assert hip.SIGNATURES['nbasr_ctc_confidence_state_bytes'] == (ctypes.c_size_t, [ctypes.c_int])
    lib = hip.load_library()
    assert lib.nbasr_ctc_confidence_step.argtypes == argtypes and lib.nbasr_version() == 6      # additive: the ABI version stays
    exported = ctypes.CDLL(str(built_library))
    assert hasattr(exported, 'nbasr_ctc_confidence_step') and hasattr(exported, 'nbasr_ctc_confidence_state_bytes')
    assert 'confidence.hip' in __import__('nb_asr_amd.build', fromlist=['SOURCES']).SOURCES
    assert hip.CONFIDENCE_STATE_WORDS == cm.STATE_WORDS == 16 and hip.CONFIDENCE_TOKEN_WORDS == cm.TOKEN_WORDS
    assert 'nbasr_ctc_confidence_step' in hip._ENQUEUES and 'nbasr_ctc_confidence_state_bytes' not in hip._ENQUEUES


def test_state_bytes():
    lib = hip.load_library()
    for batch in (1, 3, 5, 64):
        assert lib.nbasr_ctc_confidence_state_bytes(batch) == 64 * batch == hip.ctc_confidence_state_bytes(batch)
    assert [lib.nbasr_ctc_confidence_state_bytes(b) for b in (0, -1, -64)] == [0, 0, 0] and hip.ctc_confidence_state_bytes(0) == 0


def test_refusals_without_a_device():
    """Every refusal of the step happens on the host, before a launch: dummy non-NULL addresses are never touched."""
    lib = hip.load_library()
    P = 4096                                                                            # stands for a device address
    good = dict(x=P, lengths=None, path=None, state_in=P, state_out=P, measure=2, alpha=1 / 3, blank=0, final=0, tokens=P, counts=P, trace=None,
                batch=2, frames=10, classes=49)

    def call(**change):
        a = dict(good, **change)
        rc = lib.nbasr_ctc_confidence_step(a['x'], a['lengths'], a['path'], a['state_in'], a['state_out'], a['measure'], a['alpha'], a['blank'],
                                           a['final'], a['tokens'], a['counts'], a['trace'], a['batch'], a['frames'], a['classes'], None)
        return rc, lib.nbasr_last_error()

    EINVAL, ENULL = -1, -3
    for change, code, text in [
        (dict(batch=-1), EINVAL, b'negative sizes'),
        (dict(frames=-1), EINVAL, b'negative'),
        (dict(classes=1), EINVAL, b'classes=1 must lie in [2, 128]'),
        (dict(classes=129), EINVAL, b'classes'),
        (dict(blank=-1), EINVAL, b'blank=-1 must lie in [0, 49)'),
        (dict(blank=49), EINVAL, b'blank'),
        (dict(measure=3), EINVAL, b'unknown measure 3'),
        (dict(measure=-1), EINVAL, b'unknown measure'),
        (dict(alpha=0.0), EINVAL, b'alpha'),
        (dict(alpha=1.0), EINVAL, b'alpha'),
        (dict(alpha=-0.25), EINVAL, b'alpha'),
        (dict(alpha=1.5), EINVAL, b'alpha'),
        (dict(alpha=float('nan')), EINVAL, b'alpha must lie strictly between 0 and 1'),
        (dict(tokens=None), EINVAL, b'tokens_out and token_counts go together'),
        (dict(counts=None), EINVAL, b'both or neither'),
        (dict(x=None), ENULL, b'NULL'),
        (dict(state_out=None), ENULL, b'NULL'),
    ]:
        rc, message = call(**change)
        assert rc == code and text in message and b'nbasr_ctc_confidence_step' in message, (change, rc, message)
    # alpha is read by tsallis alone; nothing to do is not an error, and is decided on the host too
    assert call(batch=0, measure=0, alpha=float('nan'))[0] == 0 and call(batch=0, measure=1, alpha=7.0)[0] == 0
    assert call(batch=0)[0] == 0 and call(batch=0, x=None, frames=7)[0] == 0
    assert call(frames=0, x=None, tokens=None, counts=None)[0] == 0            # no frames, committed in place, not final, no table: nothing to launch
    assert call(batch=0, classes=2, blank=1)[0] == 0 and call(batch=0, classes=128, blank=127)[0] == 0     # the edges of the ranges are taken


# ---- the session's signature ---------------------------------------------------------------------------------------------------------
def test_session_signature():
    params = inspect.signature(streaming.StreamingSession.__init__).parameters
    names = list(params)
    assert params['confidence'].kind is inspect.Parameter.KEYWORD_ONLY and params['confidence'].default is None
    assert names[names.index('input_rate') + 1] == 'confidence' and names[names.index('confidence') + 1] == 'endpoint'
    assert names.index('endpoint') < names.index('keywords') < names.index('segments') < names.index('lm') and names[-3:] == ['lm', 'alpha', 'beta']
    assert 'confidence' not in inspect.signature(model_module.ASRModel.stream).parameters       # stream() keeps its parameter list
    assert isinstance(streaming.StreamingSession.confidence, property) and callable(streaming.StreamingSession.peek_confidence)
    assert 'provisional' in streaming.StreamingSession.peek_confidence.__doc__.lower()
    assert 'last' in streaming.StreamingSession.confidence.__doc__
