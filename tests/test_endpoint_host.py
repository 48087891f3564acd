"""The endpointer without a GPU: the definition (endpoint_model.py) on hand-written cases and its invariances, the default speech classes
and the seconds-to-frames rule, ``EndpointRules`` validation, and the C entry points' declarations, sizes and refusals."""
import ctypes

import numpy as np
import pytest

from nb_asr_amd import ctc, hip, phonemes
from nbasr_header import declarations
import endpoint_model as em

S2 = (1,)                        # two classes: 0 = non-speech, 1 = speech
SPEECH, QUIET = (0.0, 1.0), (1.0, 0.0)


def frames_of(pattern):
    """'s' = a speech frame, '.' = a non-speech one -> (1, n, 2) float32."""
    return np.array([[SPEECH if ch == 's' else QUIET for ch in pattern]], dtype=np.float32).reshape(1, len(pattern), 2)


def run(pattern, rules, margin=0.0):
    state, mask = em.step(frames_of(pattern), None, None, rules, S2, margin)
    return tuple(int(v) for v in state[0]), ''.join('s' if m else '.' for m in mask[0])


# ---- the model ---------------------------------------------------------------------------------------------------------------------
def test_hand_written_cases():
    # (frames, speech_frames, first_speech, last_speech, endpoint_frame, endpoint_rule, 0, 0)
    assert run('', ((0, 1, 0),)) == ((0, 0, -1, -1, -1, -1, 0, 0), '')
    assert em.fresh(2).tolist() == [[0, 0, -1, -1, -1, -1, 0, 0]] * 2
    # nothing said: trailing counts every frame, so 3 frames of silence end it at frame 2
    assert run('....', ((0, 3, 0),)) == ((4, 0, -1, -1, 2, 0, 0, 0), '....')
    # speech at 1 and 2, then silence: trailing = g - last_speech reaches 2 at frame 4
    assert run('.ss...', ((1, 2, 0),)) == ((6, 2, 1, 2, 4, 0, 0, 0), '.ss...')
    # the same rule never holds without speech; the length rule does, at frame 4 (n_seen = 5)
    assert run('......', ((1, 2, 0), (0, 0, 5))) == ((6, 0, -1, -1, 4, 1, 0, 0), '......')
    # a rule of zeros holds at the first frame
    assert run('s.', ((0, 0, 0),)) == ((2, 1, 0, 0, 0, 0, 0, 0), 's.')
    # min_speech counts frames, not runs
    assert run('s.s.s', ((3, 0, 0),)) == ((5, 3, 0, 4, 4, 0, 0, 0), 's.s.s')
    # no rule holds: no endpoint
    assert run('ssss', ((1, 1, 0),)) == ((4, 4, 0, 3, -1, -1, 0, 0), 'ssss')


def test_the_endpoint_latches_and_the_counters_go_on():
    state = run('s..s.....', ((1, 2, 0), (0, 0, 1)))[0]
    # rule 1 (one frame in all) holds at frame 0 already and stays: later frames at which rule 0 holds change nothing
    assert state == (9, 2, 0, 3, 0, 1, 0, 0)
    assert run('s..s.....', ((1, 2, 0),))[0] == (9, 2, 0, 3, 2, 0, 0, 0)      # latched at 2; speech at 3 and silence to 8 do not move it


def test_the_lowest_rule_wins_a_tie():
    # at frame 3 both rules hold for the first time (trailing = 2; n_seen = 4)
    assert run('.s....', ((1, 2, 0), (0, 0, 4)))[0][4:6] == (3, 0)
    assert run('.s....', ((0, 0, 4), (1, 2, 0)))[0][4:6] == (3, 0)
    assert run('.s....', ((9, 0, 0), (0, 0, 4), (1, 2, 0)))[0][4:6] == (3, 1)


def test_margin_ties_and_nan():
    tie = np.array([[[2.0, 2.0]]], dtype=np.float32)
    assert em.step(tie, None, None, ((0, 0, 9),), S2, 0.0)[1].tolist() == [[0]]          # ms > mn is false on a tie
    x = np.array([[[1.0, 1.5], [1.0, 1.25], [np.nan, 5.0], [5.0, np.nan], [np.nan, np.nan], [-np.inf, 0.0]]], dtype=np.float32)
    assert em.step(x, None, None, ((0, 0, 9),), S2, 0.0)[1].tolist() == [[1, 1, 1, 0, 0, 1]]
    assert em.step(x, None, None, ((0, 0, 9),), S2, 0.5)[1].tolist() == [[0, 0, 1, 0, 0, 1]]   # 1.5 > 1.0 + 0.5 is false
    # a NaN is never taken: a frame whose speech classes are all NaN is non-speech, whatever the rest holds
    assert not em.is_speech(np.array([0.0, np.nan, np.nan], dtype=np.float32), (1, 2), 0.0)
    assert em.is_speech(np.array([np.nan, -3.0, np.nan], dtype=np.float32), (1, 2), 0.0)       # (no other class is a number: mn = -inf)


def random_case(seed, classes=9):
    rng = np.random.default_rng(seed)
    n, batch = int(rng.integers(1, 90)), int(rng.integers(1, 4))
    x = rng.standard_normal((batch, n, classes)).astype(np.float32)
    x[rng.random((batch, n)) < 0.5, 0] += 3.0                                  # class 0 (non-speech) wins about half the frames
    speech = tuple(sorted(rng.choice(np.arange(1, classes), size=int(rng.integers(1, classes - 1)), replace=False).tolist()))
    rules = tuple(tuple(int(v) for v in rng.integers(0, (8, 6, 60))) for _ in range(int(rng.integers(1, 5))))
    lengths = rng.integers(0, n + 1, size=batch)
    return x, lengths, rules, speech


@pytest.mark.parametrize('seed', range(20))
def test_a_shift_of_a_frame_changes_nothing(seed):
    """x + k per frame, k a power of two times an integer small enough that every sum is exact in float32: the same decisions at margin 0
    and at a margin that is itself such a number."""
    x, lengths, rules, speech = random_case(seed)
    x = np.round(x * 64) / 64                                                   # multiples of 2^-6 below 2^4
    shift = np.random.default_rng(seed + 100).integers(-512, 512, size=x.shape[:2]).astype(np.float32)[..., None] / 8
    for margin in (0.0, 0.25):
        a = em.step(x, lengths, None, rules, speech, margin)
        b = em.step((x + shift).astype(np.float32), lengths, None, rules, speech, margin)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize('seed', range(30))
def test_any_chunking_equals_the_whole(seed):
    x, lengths, rules, speech = random_case(seed)
    whole, mask = em.step(x, lengths, None, rules, speech, 0.0)
    rng = np.random.default_rng(seed + 1000)
    state, at, masks = None, 0, []
    n = x.shape[1]
    while at < n:
        k = int(rng.integers(0, 40))
        k = min(k, n - at)
        state, m = em.step(x[:, at:at + k], np.clip(lengths - at, 0, k), state, rules, speech, 0.0)
        masks.append(m)
        at += k
    assert np.array_equal(state, whole) and np.array_equal(np.concatenate(masks, 1), mask)
    assert not whole[:, 6:].any()
    assert np.array_equal(whole[:, 0], lengths) and np.array_equal(whole[:, 1], mask.sum(1))


# ---- the defaults and from_seconds -------------------------------------------------------------------------------------------------
def test_default_speech_classes():
    speech = ctc.default_speech_classes()
    assert set(range(49)) - set(speech) == {0, 10, 17, 38, 44} and list(speech) == sorted(speech) and len(speech) == 44
    names = phonemes.vocab(48, inc_blank=True)
    assert [names[i] for i in (0, 10, 17, 38, 44)] == ['_', 'cl', 'epi', 'sil', 'vcl']
    rules = ctc.EndpointRules()
    assert rules.speech_classes == speech and rules.classes == 49 and rules.margin == 0.0
    assert rules.rules == ((0, 125, 0), (1, 25, 0), (0, 0, 500))
    word = rules.speech_lo | (rules.speech_hi << 64)
    assert [c for c in range(128) if word >> c & 1] == list(speech) and rules.speech_hi == 0


def test_from_seconds():
    assert ctc.FRAME_SECONDS == 0.04
    assert [ctc.EndpointRules.frames_for(s) for s in (1.0, 0.05, 0.0, 0.04, 0.041, 0.0404, 5.0, 20.0, 0.08, 0.081)] == [25, 2, 0, 1, 2, 1, 125, 500, 2, 3]
    assert ctc.EndpointRules.from_seconds().rules == ctc.EndpointRules().rules
    assert ctc.EndpointRules.from_seconds(((0.5, 0.05, 0), (0, 0, 1.0)), margin=1.5).rules == ((13, 2, 0), (0, 0, 25))
    assert ctc.EndpointRules.from_seconds(((0, 1, 0),), margin=1.5).margin == 1.5
    with pytest.raises(ValueError, match='negative'):
        ctc.EndpointRules.from_seconds(((0, -0.1, 0),))


def test_rules_in_both_words_of_the_mask():
    rules = ctc.EndpointRules(((0, 1, 0),), speech_classes=(1, 63, 64, 99), classes=100)
    assert rules.speech_lo == (1 << 1) | (1 << 63) and rules.speech_hi == 1 | (1 << 35)
    assert hip._signed64(rules.speech_lo) < 0 and hip._signed64(rules.speech_lo) & (2 ** 64 - 1) == rules.speech_lo


@pytest.mark.parametrize('kwargs,match', [
    (dict(classes=1, speech_classes=(0,)), 'classes'),
    (dict(classes=129, speech_classes=(0,)), 'classes'),
    (dict(classes=50), 'speech_classes must be given'),
    (dict(speech_classes=()), 'empty'),
    (dict(speech_classes=range(49)), 'every class'),
    (dict(speech_classes=(1, 49)), r'lie in \[0, 49\)'),
    (dict(speech_classes=(-1, 3)), r'lie in \[0, 49\)'),
    (dict(speech_classes=(3, 3)), 'twice'),
    (dict(rules=()), 'rules'),
    (dict(rules=((0, 1, 0),) * 9), 'rules'),
    (dict(rules=((0, 1),)), 'a rule is'),
    (dict(rules=((0, -1, 0),)), 'a rule is'),
    (dict(rules=((0, 1.5, 0),)), 'a rule is'),
    (dict(rules=((0, 2 ** 31, 0),)), 'a rule is'),
    (dict(margin=-0.5), 'margin'),
    (dict(margin=float('nan')), 'margin'),
    (dict(device='cpu'), 'HIP device'),
])
def test_rules_validation(kwargs, match):
    with pytest.raises(ValueError, match=match):
        ctc.EndpointRules(**kwargs)


def test_streams_and_sessions_refuse_what_is_not_a_rule_set():
    with pytest.raises(ValueError, match='batch'):
        ctc.EndpointStream(0, ctc.EndpointRules())
    with pytest.raises(ValueError, match='EndpointRules'):
        ctc.EndpointStream(1, ((0, 1, 0),))
    with pytest.raises(ValueError, match='HIP device'):
        ctc.EndpointStream(1, ctc.EndpointRules(), device='cpu')
    with pytest.raises(ValueError, match='EndpointRules'):
        ctc.endpoint(np.zeros((1, 2, 49), dtype=np.float32), rules=((0, 1, 0),))
    import torch
    with pytest.raises(ValueError, match='HIP device'):
        ctc.endpoint(torch.zeros(1, 2, 49))
    with pytest.raises(ValueError, match='classes'):
        ctc.endpoint(torch.zeros(1, 2, 48))


# ---- the C entry points ------------------------------------------------------------------------------------------------------------
def test_header_and_binding_entries():
    decl = declarations()
    assert decl['nbasr_ctc_endpoint_state_bytes'] == ('size_t', ['int batch'])
    ret, params = decl['nbasr_ctc_endpoint_step']
    assert ret == 'int'
    assert [p.rsplit(' ', 1)[1].lstrip('*') for p in params] == ['x', 'lengths', 'state_in', 'state_out', 'rules', 'n_rules', 'speech_lo', 'speech_hi',
                                                                'margin', 'mask_out', 'batch', 'frames', 'classes', 'stream']
    assert params[2].startswith('const int*') and params[3] == 'int* state_out'        # a peek's input state is const
    restype, argtypes = hip.SIGNATURES['nbasr_ctc_endpoint_step']
    assert restype is ctypes.c_int and len(argtypes) == 14
    assert argtypes[6] is argtypes[7] is ctypes.c_longlong and argtypes[8] is ctypes.c_float
    assert hip.load_library().nbasr_version() == 6                                     # additive: the ABI version stays


def test_state_bytes():
    lib = hip.load_library()
    assert [lib.nbasr_ctc_endpoint_state_bytes(b) for b in (1, 5, 64, 0, -3)] == [32, 160, 2048, 0, 0]
    assert hip.ctc_endpoint_state_bytes(16) == 16 * hip.ENDPOINT_STATE_WORDS * 4 == 16 * em.STATE_WORDS * 4


def test_refusals_without_a_device():
    """Every refusal of the step happens on the host, before a launch: dummy non-NULL addresses are never touched."""
    lib = hip.load_library()
    P = 4096                                                                            # stands for a device address
    good = dict(x=P, lengths=None, state_in=P, state_out=P, rules=P, n_rules=3, lo=0b1010, hi=0, margin=0.0, mask=None, batch=2, frames=10,
                classes=49)

    def call(**change):
        a = dict(good, **change)
        rc = lib.nbasr_ctc_endpoint_step(a['x'], a['lengths'], a['state_in'], a['state_out'], a['rules'], a['n_rules'], hip._signed64(a['lo']),
                                         hip._signed64(a['hi']), a['margin'], a['mask'], a['batch'], a['frames'], a['classes'], None)
        return rc, lib.nbasr_last_error()

    EINVAL, ENULL = -1, -3
    for change, code, text in [
        (dict(x=None), ENULL, b'NULL'),
        (dict(state_out=None), ENULL, b'NULL'),
        (dict(rules=None), ENULL, b'NULL'),
        (dict(classes=1), EINVAL, b'classes'),
        (dict(classes=129), EINVAL, b'classes'),
        (dict(lo=0), EINVAL, b'empty'),
        (dict(lo=(1 << 49) - 1), EINVAL, b'every class'),
        (dict(classes=64, lo=2 ** 64 - 1), EINVAL, b'every class'),
        (dict(classes=128, lo=2 ** 64 - 1, hi=2 ** 64 - 1), EINVAL, b'every class'),
        (dict(classes=100, lo=2 ** 64 - 1, hi=(1 << 36) - 1), EINVAL, b'every class'),
        (dict(lo=1 << 49), EINVAL, b'at or above'),
        (dict(hi=1), EINVAL, b'at or above'),
        (dict(classes=64, lo=1, hi=1), EINVAL, b'at or above'),
        (dict(classes=100, lo=1, hi=1 << 36), EINVAL, b'at or above'),
        (dict(n_rules=0), EINVAL, b'n_rules'),
        (dict(n_rules=9), EINVAL, b'n_rules'),
        (dict(margin=-1.0), EINVAL, b'margin'),
        (dict(margin=float('nan')), EINVAL, b'margin'),
        (dict(batch=-1), EINVAL, b'negative'),
        (dict(frames=-1), EINVAL, b'negative'),
    ]:
        rc, message = call(**change)
        assert rc == code and text in message, (change, rc, message)
    # nothing to do is not an error, and is decided on the host too: an empty batch; no frames with the state committed in place
    assert call(batch=0)[0] == 0
    assert call(frames=0, x=None)[0] == 0
    assert call(batch=0, x=None, frames=7)[0] == 0
