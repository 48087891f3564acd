"""The keyword spotter without a GPU: the definition (keyword_model.py) against brute force over every start and every frame labelling,
its properties and invariances, the NaN behaviour as defined, ``KeywordSet`` validation and ``from_phonemes``, the C entry points'
declarations, sizes and refusals, and the session's signature."""
import ctypes
import functools
import inspect
import itertools

import numpy as np
import pytest
import torch

from nb_asr_amd import ctc, hip, model as model_module, phonemes, streaming
from nbasr_header import declarations
import keyword_model as km

BLANK = 0
A, B, C = 1, 2, 3


def run(x, keywords, thresholds=None, lengths=None, state=None):
    """The model on one utterance (n, C) or a batch (B, n, C)."""
    x = np.asarray(x, dtype=np.float32)
    x = x[None] if x.ndim == 2 else x
    thresholds = [-1e30] * len(keywords) if thresholds is None else thresholds
    return km.step(x, lengths, state, keywords, thresholds, BLANK)


def greedy_frames(labels, classes=4, high=2.0):
    """(n, classes) float32 whose per-frame maximum is at ``labels``: `high` there, 0 elsewhere (a frame off the path costs -high)."""
    x = np.zeros((len(labels), classes), dtype=np.float32)
    x[np.arange(len(labels)), labels] = high
    return x


# ---- the model against brute force ---------------------------------------------------------------------------------------------------
def collapse(labels):
    out, prev = [], None
    for v in labels:
        if v != prev and v != BLANK:
            out.append(v)
        prev = v
    return tuple(out)


@functools.lru_cache(maxsize=None)
def labellings(classes, keyword, n):
    """Every labelling of n frames that begins on the keyword's first token, ends on its last and CTC-collapses to it: (count, n)."""
    rows = [p for p in itertools.product(range(classes), repeat=n) if p[0] == keyword[0] and p[-1] == keyword[-1] and collapse(p) == keyword]
    return np.array(rows, dtype=np.int64).reshape(len(rows), n)


def brute(x, keyword):
    """best[f, g]: the largest sum of x[t, label] - max(x[t]) over the labellings of frames f..g (-inf: there is none)."""
    n, classes = x.shape
    d = x.astype(np.float64) - x.astype(np.float64).max(1, keepdims=True)
    best = np.full((n, n), -np.inf)
    for f in range(n):
        for g in range(f, n):
            rows = labellings(classes, keyword, g - f + 1)
            if len(rows):
                best[f, g] = d[np.arange(f, g + 1)[None, :], rows].sum(1).max()
    return best


BRUTE_CASES = [(classes, keyword, seed) for classes in (2, 3, 4) for length in (1, 2, 3)
               for keyword in itertools.product(range(1, classes), repeat=length) for seed in range(4)]


def test_the_model_equals_brute_force_over_every_start_and_labelling():
    """Inputs on a grid of 1/8, so every float32 sum is exact: the scores are equal exactly, the reported start is a maximising one."""
    assert len(BRUTE_CASES) == 4 * (3 + 14 + 39)
    compared = 0
    for classes, keyword, seed in BRUTE_CASES:
        rng = np.random.default_rng(hash((classes, keyword, seed)) % 2 ** 32)
        n = int(rng.integers(1, 7)) if seed < 2 else 6
        x = (rng.integers(-16, 17, size=(n, classes)) / 8).astype(np.float32)
        if seed % 2:
            x[rng.random(n) < 0.6, 0] += 1.0                                            # blank-dominated frames, as a CTC model's
        want = brute(x, keyword)
        _, scores, starts = run(x, [keyword])
        for g in range(n):
            column = want[:g + 1, g]
            assert scores[0, 0, g] == column.max(), (classes, keyword, seed, g, scores[0, 0], want)
            if np.isfinite(column.max()):
                assert 0 <= starts[0, 0, g] <= g and column[starts[0, 0, g]] == column.max(), (classes, keyword, seed, g)
                compared += 1
            else:
                assert starts[0, 0, g] == -1
            # 2 L - 1 frames hold any keyword of L tokens (a blank between repeats): from there on there is a path
            assert np.isfinite(column.max()) or g < 2 * len(keyword) - 2
    assert compared >= 2 * len(BRUTE_CASES)                        # (the cases of 6 frames alone: frames 4 and 5 at the least)


# ---- properties ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('seed', range(10))
def test_a_score_is_never_positive(seed):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((3, 40, 7)) * 4).astype(np.float32)
    keywords = [tuple(rng.integers(1, 7, size=int(rng.integers(1, 6))).tolist()) for _ in range(4)]
    state, scores, _ = run(x, keywords)
    assert (scores <= 0).all() and (km.fields(state)['best_score'] <= 0).all()


def test_the_score_is_zero_with_the_right_span_when_the_greedy_path_spells_the_keyword():
    #         0  1  2  3  4  5  6  7  8  9
    labels = [0, C, 0, A, A, 0, B, B, C, 0]
    state, scores, starts = run(greedy_frames(labels), [(A, B), (A, B, C), (B,), (C, A)], thresholds=[0.0] * 4)
    f = km.fields(state)
    assert scores[0, 0].tolist() == [-np.inf, -4, -4, -4, -2, -2, 0, 0, -2, -4] and starts[0, 0, 4:].tolist() == [3] * 6       # (frame 0: no path yet)
    assert scores[0, 1, 8] == 0 and starts[0, 1, 8] == 3 and (scores[0, 1, :8] < 0).all() and scores[0, 1, 9] < 0
    assert f['hit_frame'][0].tolist() == [6, 8, 6, 3] and f['hit_start'][0].tolist() == [3, 3, 6, 1] and (f['hit_score'][0] == 0).all()
    assert f['best_frame'][0].tolist() == [6, 8, 6, 3] and f['best_start'][0].tolist() == [3, 3, 6, 1]      # the earliest frame of a tie
    assert f['frames'][0].tolist() == [10] * 4


def test_a_repeated_token_needs_the_blank_between():
    together, apart = greedy_frames([A, A, A, A]), greedy_frames([A, A, 0, A])
    assert run(together, [(A, A)])[1][0, 0].tolist() == [-np.inf, -np.inf, -2, -2]     # a frame has to be the blank: it costs 2
    _, scores, starts = run(apart, [(A, A)])
    assert scores[0, 0].tolist() == [-np.inf, -np.inf, -4, 0] and starts[0, 0, 2:].tolist() == [0, 0]     # (three frames at the least)
    # two different tokens need none
    assert run(greedy_frames([A, A, B, B]), [(A, B)])[1][0, 0].tolist() == [-np.inf, -2, 0, 0]
    assert km.states_of((A, A, B), BLANK) == [A, BLANK, A, BLANK, B]


def test_the_hit_latches_and_the_best_goes_on_improving():
    weak = greedy_frames([0, A, C, 0], high=1.0)                  # "a b" with the b frame won by c: costs 1
    strong = greedy_frames([0, A, B, 0], high=1.0)
    x = np.concatenate([weak, strong, weak])
    state, scores, _ = run(x, [(A, B)], thresholds=[-1.5])
    f = km.fields(state)
    assert scores[0, 0, 2] == -1 and scores[0, 0, 6] == 0
    assert (f['hit_frame'][0, 0], f['hit_start'][0, 0], f['hit_score'][0, 0]) == (2, 1, -1)          # the first frame at or above -1.5
    assert (f['best_frame'][0, 0], f['best_start'][0, 0], f['best_score'][0, 0]) == (6, 5, 0)        # ... and the best since
    # score >= threshold: equality hits; just below does not
    assert km.fields(run(x, [(A, B)], thresholds=[-1.0])[0])['hit_frame'][0, 0] == 2
    assert km.fields(run(x, [(A, B)], thresholds=[-0.5])[0])['hit_frame'][0, 0] == 6
    never = km.fields(run(weak, [(A, B)], thresholds=[-0.5])[0])
    assert never['hit_frame'][0, 0] == -1 and never['hit_start'][0, 0] == -1 and never['hit_score'][0, 0] == -np.inf
    assert never['best_frame'][0, 0] == 2


def random_case(seed, classes=6):
    rng = np.random.default_rng(seed)
    n, batch = int(rng.integers(1, 70)), int(rng.integers(1, 4))
    x = (rng.integers(-24, 25, size=(batch, n, classes)) / 8).astype(np.float32)
    x[rng.random((batch, n)) < 0.4, 0] += 2.0
    keywords = [tuple(rng.integers(1, classes, size=int(rng.integers(1, 5))).tolist()) for _ in range(int(rng.integers(1, 4)))]
    thresholds = (-rng.integers(0, 24, size=len(keywords)) / 8).tolist()
    lengths = rng.integers(0, n + 1, size=batch)
    return x, lengths, keywords, thresholds


@pytest.mark.parametrize('seed', range(20))
def test_any_chunking_equals_the_whole(seed):
    x, lengths, keywords, thresholds = random_case(seed)
    whole, scores, starts = km.step(x, lengths, None, keywords, thresholds, BLANK)
    rng = np.random.default_rng(seed + 1000)
    state, at, parts = None, 0, []
    n = x.shape[1]
    while at < n:
        k = min(int(rng.integers(0, 30)), n - at)
        state, s, f = km.step(x[:, at:at + k], np.clip(lengths - at, 0, k), state, keywords, thresholds, BLANK)
        parts.append((s, f))
        at += k
    assert np.array_equal(state, whole)
    assert np.array_equal(np.concatenate([p[0] for p in parts], 2), scores) and np.array_equal(np.concatenate([p[1] for p in parts], 2), starts)
    assert np.array_equal(whole[:, :, 0], np.repeat(lengths[:, None], len(keywords), 1)) and not whole[:, :, 7].any()
    for k, word in enumerate(keywords):                           # states at or above S hold -inf and -1
        S = 2 * len(word) - 1
        assert (whole[:, k, 8 + S:72] == km.NEG_INF_BITS).all() and (whole[:, k, 72 + S:] == -1).all()
    for b in range(x.shape[0]):                                   # beyond a row's length: -inf and -1
        assert np.isneginf(scores[b, :, lengths[b]:]).all() and (starts[b, :, lengths[b]:] == -1).all()


@pytest.mark.parametrize('seed', range(10))
def test_a_shift_of_a_frame_changes_nothing(seed):
    """x + k per frame with every sum exact in float32 (a grid of 1/8): logits and log-probabilities give the same costs."""
    x, lengths, keywords, thresholds = random_case(seed)
    shift = np.random.default_rng(seed + 100).integers(-512, 512, size=x.shape[:2]).astype(np.float32)[..., None] / 8
    a, b = km.step(x, lengths, None, keywords, thresholds, BLANK), km.step((x + shift).astype(np.float32), lengths, None, keywords, thresholds, BLANK)
    assert all(np.array_equal(p, q) for p, q in zip(a, b))


# ---- NaN -----------------------------------------------------------------------------------------------------------------------------
def test_nan_behaviour_is_the_defined_one():
    x, _, _, _ = random_case(3)
    x = x[:1, :, :]
    n = x.shape[1]
    assert n > 12
    keywords, at = [(A, B), (C,), (B, B, A)], 7
    clean = run(x, keywords)
    # a NaN in a class no keyword holds is never taken by the maximum: the frame is what it is without that class
    ignored = x.copy()
    ignored[0, at, 4] = np.nan
    assert (x[0, at].argmax() != 4) and all(np.array_equal(p, q) for p, q in zip(run(ignored, keywords), clean))
    # a NaN in token A's column makes V'[s] NaN in the states of A at that frame only; keyword (C,) never sees it
    poisoned = x.copy()
    poisoned[0, at, A] = np.nan
    state, scores, starts = run(poisoned, keywords)
    assert np.array_equal(scores[0, 1], clean[1][0, 1]) and np.array_equal(starts[0, 1], clean[2][0, 1])
    assert np.isnan(scores[0, 2, at]) and not np.isnan(scores[0, 2, at + 1:]).any() and not np.isnan(scores[0, 0]).any()
    assert not np.isnan(state[:, :, 8:72].view(np.float32)).any()                     # the NaN is never taken again: it is gone a frame later
    # a frame of NaN alone: m stays -inf, every x[z(s)] - m is NaN, every path through the frame dies; what follows is a fresh run of
    # the frames after it (the starts are global frame indices), and neither the hit nor the best takes a NaN
    dead = x.copy()
    dead[0, at, :] = np.nan
    state, scores, starts = run(dead, keywords, thresholds=[0.0] * 3)
    assert np.isnan(scores[0, :, at]).all()
    _, tail_scores, tail_starts = run(x[:, at + 1:], keywords)
    assert np.array_equal(scores[:, :, at + 1:], tail_scores)
    assert np.array_equal(starts[:, :, at + 1:], np.where(tail_starts >= 0, tail_starts + at + 1, -1))
    f = km.fields(state)
    assert not np.isnan(f['best_score']).any() and not np.isnan(f['hit_score']).any() and (f['best_frame'] != at).all() and (f['frames'] == n).all()
    head = km.fields(run(x[:, :at], keywords)[0])
    assert (f['best_score'] >= head['best_score']).all()


# ---- KeywordSet ----------------------------------------------------------------------------------------------------------------------
def test_keyword_set_defaults_and_tables():
    ks = ctc.KeywordSet([[3, 4], (5,), range(1, 33)])
    assert len(ks) == 3 and ks.keywords == ((3, 4), (5,), tuple(range(1, 33))) and ks.classes == 49 and ks.blank == 0
    assert ks.thresholds == (-2.0, -1.0, -32.0)                   # -per_token * L, per_token = 1: untuned
    assert ctc.KeywordSet([[3, 4], [5]], per_token=0.5).thresholds == (-1.0, -0.5)
    assert ctc.KeywordSet([[3, 4], [5]], thresholds=-3).thresholds == (-3.0, -3.0)
    assert ctc.KeywordSet([[3, 4], [5]], thresholds=[-0.25, 0.0]).thresholds == (-0.25, 0.0)
    assert ctc.KeywordSet([[0, 2]], classes=3, blank=1).keywords == ((0, 2),)
    tokens, counts, thresholds = ks.host_tables()
    assert tokens.shape == (3, 32) and tokens.dtype == torch.int32 and counts.tolist() == [2, 1, 32] and thresholds.dtype == torch.float32
    assert tokens[0].tolist() == [3, 4] + [-1] * 30 and tokens[2].tolist() == list(range(1, 33))
    assert 'UNTUNED' in ctc.KeywordSet.__doc__


def test_from_phonemes():
    names = phonemes.vocab(48, inc_blank=True)
    ks = ctc.KeywordSet.from_phonemes([['sh', 'iy'], ['sil']], thresholds=[-1.0, -2.0])
    assert ks.keywords == ((names.index('sh'), names.index('iy')), (names.index('sil'),)) and ks.classes == 49 and ks.blank == 0
    assert ks.thresholds == (-1.0, -2.0) and ctc.KeywordSet.from_phonemes([['sh', 'iy']], per_token=2).thresholds == (-4.0,)
    for bad in ([['sh', 'xx']], [[names[0]]], ['sh']):
        with pytest.raises(ValueError, match='phoneme'):
            ctc.KeywordSet.from_phonemes(bad)


@pytest.mark.parametrize('args,kwargs,match', [
    (([],), {}, '1 to 64 keywords'),
    (([[1]] * 65,), {}, '1 to 64 keywords'),
    (([[]],), {}, '1 to 32 tokens'),
    (([[1] * 33],), {}, '1 to 32 tokens'),
    (([[1, 49]],), {}, r'lie in \[0, 49\)'),
    (([[-1]],), {}, r'lie in \[0, 49\)'),
    (([[1, 0]],), {}, 'blank'),
    (([[1, 2]],), dict(blank=2), 'blank'),
    (([[1.5]],), {}, 'token ids'),
    (([1, 2],), {}, 'sequence of token ids'),
    ((['ab'],), {}, 'sequence of token ids'),
    ((3,), {}, 'sequence of token-id sequences'),
    (([[1]],), dict(thresholds=[0.5]), 'threshold'),
    (([[1]],), dict(thresholds=[float('nan')]), 'threshold'),
    (([[1]],), dict(thresholds=[float('-inf')]), 'threshold'),
    (([[1]],), dict(thresholds=[-1e39]), 'threshold'),             # -inf once it is the float32 the kernel compares with
    (([[1]],), dict(thresholds=[-1.0, -1.0]), 'expected 1 thresholds'),
    (([[1]],), dict(per_token=-1.0), 'per_token'),
    (([[1]],), dict(per_token=float('inf')), 'per_token'),
    (([[1]],), dict(classes=1), 'classes'),
    (([[1]],), dict(classes=129), 'classes'),
    (([[1]],), dict(blank=49), r'blank must lie'),
    (([[1]],), dict(device='cpu'), 'HIP device'),
])
def test_keyword_set_validation(args, kwargs, match):
    with pytest.raises(ValueError, match=match):
        ctc.KeywordSet(*args, **kwargs)


def test_functions_streams_and_sessions_refuse_without_a_device():
    ks = ctc.KeywordSet([[1, 2]])
    with pytest.raises(ValueError, match='batch'):
        ctc.KeywordStream(0, ks)
    with pytest.raises(ValueError, match='KeywordSet'):
        ctc.KeywordStream(1, [[1, 2]])
    with pytest.raises(ValueError, match='HIP device'):
        ctc.KeywordStream(1, ks, device='cpu')
    with pytest.raises(ValueError, match='KeywordSet'):
        ctc.spot_keywords(torch.zeros(1, 2, 49))
    with pytest.raises(ValueError, match='KeywordSet'):
        ctc.spot_keywords(torch.zeros(1, 2, 49), keywords=[[1, 2]])
    with pytest.raises(ValueError, match='HIP device'):
        ctc.spot_keywords(torch.zeros(1, 2, 49), keywords=ks)
    with pytest.raises(ValueError, match='classes'):
        ctc.spot_keywords(torch.zeros(1, 2, 48), keywords=ks)
    with pytest.raises(ValueError, match='expected'):
        ctc.spot_keywords(torch.zeros(2, 49), keywords=ks)
    with pytest.raises(ValueError, match='KeywordSet'):
        streaming.StreamingSession(None, 1, keywords=[[1, 2]])        # refused before the model is looked at
    with pytest.raises(hip.HipError, match='HIP device'):
        hip.ctc_keyword_step(torch.zeros(1, 2, 49), None, *ks.host_tables(), 0, None, torch.zeros(1, 1, 136, dtype=torch.int32))


def test_a_result_names_the_words_of_its_state():
    state = torch.from_numpy(km.fresh(2, 3))
    state[1, 2, :8] = torch.tensor([9, 4, 2, 0, 7, 5, 0, 0], dtype=torch.int32)
    state[1, 2, 3] = int(np.array(-0.5, dtype=np.float32).view(np.int32))
    state[1, 2, 6] = int(np.array(-0.25, dtype=np.float32).view(np.int32))
    r = ctc.KeywordResult(state)
    for name, want in km.fields(state.numpy()).items():
        got = getattr(r, name)
        assert got.shape == (2, 3) and got.dtype == (torch.float32 if 'score' in name else torch.int32)
        assert np.array_equal(got.numpy(), want), name
        assert got.untyped_storage().data_ptr() == state.untyped_storage().data_ptr()  # views of the state: no copy
    assert r.detected.tolist() == [[False] * 3, [False, False, True]]
    hit_start, hit_end, best_start, best_end = r.seconds()
    assert ctc.FRAME_SECONDS == 0.04
    assert hit_start[1, 2].item() == pytest.approx(0.08) and hit_end[1, 2].item() == pytest.approx(0.2)
    assert best_start[1, 2].item() == pytest.approx(0.2) and best_end[1, 2].item() == pytest.approx(0.32)
    assert hit_start[0, 0].item() == hit_end[0, 0].item() == best_start[0, 0].item() == best_end[0, 0].item() == -1.0
    kept = r.clone()
    state[1, 2, 1] = -1
    assert kept.hit_frame[1, 2].item() == 4 and r.hit_frame[1, 2].item() == -1
    assert np.array_equal(ctc._fresh_keyword_state(2, 3).numpy(), km.fresh(2, 3))
    assert sorted(ctc.KeywordResult.FIELDS) == sorted(list(km.INT_FIELDS) + list(km.FLOAT_FIELDS))


# ---- the C entry points --------------------------------------------------------------------------------------------------------------
def test_header_and_binding_entries():
    decl = declarations()
    assert decl['nbasr_ctc_keyword_state_bytes'] == ('size_t', ['int batch', 'int n_keywords'])
    ret, params = decl['nbasr_ctc_keyword_step']
    assert ret == 'int'
    assert [p.rsplit(' ', 1)[1].lstrip('*') for p in params] == ['x', 'lengths', 'tokens', 'token_counts', 'thresholds', 'n_keywords', 'blank',
                                                                'state_in', 'state_out', 'scores_out', 'starts_out', 'batch', 'frames', 'classes',
                                                                'stream']
    assert params[0].startswith('const float*') and params[4].startswith('const float*')
    assert all(params[i].startswith('const int*') for i in (1, 2, 3, 7))               # a peek's input state is const
    assert params[8] == 'int* state_out' and params[9] == 'float* scores_out' and params[10] == 'int* starts_out'
    restype, argtypes = hip.SIGNATURES['nbasr_ctc_keyword_step']
    assert restype is ctypes.c_int and len(argtypes) == 15
    assert all(argtypes[i] is ctypes.c_int for i in (5, 6, 11, 12, 13)) and all(argtypes[i] is ctypes.c_void_p for i in (0, 1, 2, 3, 4, 7, 8, 9, 10))
    restype, argtypes = hip.SIGNATURES['nbasr_ctc_keyword_state_bytes']
    assert restype is ctypes.c_size_t and argtypes == [ctypes.c_int, ctypes.c_int]
    lib = hip.load_library()
    assert lib.nbasr_version() == 6                                                    # additive: the ABI version stays
    assert lib.nbasr_ctc_keyword_step.argtypes == hip.SIGNATURES['nbasr_ctc_keyword_step'][1]


def test_state_bytes():
    lib = hip.load_library()
    assert [lib.nbasr_ctc_keyword_state_bytes(b, k) for b, k in ((1, 1), (5, 3), (16, 64), (0, 3), (3, 0), (-3, 2))] == [544, 8160, 557056, 0, 0, 0]
    assert hip.ctc_keyword_state_bytes(16, 8) == 16 * 8 * hip.KEYWORD_STATE_WORDS * 4 == 16 * 8 * km.STATE_WORDS * 4
    assert hip.KEYWORD_STATE_WORDS == 136


def test_refusals_without_a_device():
    """Every refusal of the step happens on the host, before a launch: dummy non-NULL addresses are never touched."""
    lib = hip.load_library()
    P = 4096                                                                            # stands for a device address
    good = dict(x=P, lengths=None, tokens=P, counts=P, thresholds=P, n_keywords=3, blank=0, state_in=P, state_out=P, scores=None, starts=None,
                batch=2, frames=10, classes=49)

    def call(**change):
        a = dict(good, **change)
        rc = lib.nbasr_ctc_keyword_step(a['x'], a['lengths'], a['tokens'], a['counts'], a['thresholds'], a['n_keywords'], a['blank'],
                                        a['state_in'], a['state_out'], a['scores'], a['starts'], a['batch'], a['frames'], a['classes'], None)
        return rc, lib.nbasr_last_error()

    EINVAL, ENULL = -1, -3
    for change, code, text in [
        (dict(x=None), ENULL, b'NULL'),
        (dict(tokens=None), ENULL, b'NULL'),
        (dict(counts=None), ENULL, b'NULL'),
        (dict(thresholds=None), ENULL, b'NULL'),
        (dict(state_out=None), ENULL, b'NULL'),
        (dict(classes=1), EINVAL, b'classes'),
        (dict(classes=129), EINVAL, b'classes'),
        (dict(n_keywords=0), EINVAL, b'n_keywords'),
        (dict(n_keywords=65), EINVAL, b'n_keywords'),
        (dict(blank=-1), EINVAL, b'blank'),
        (dict(blank=49), EINVAL, b'blank'),
        (dict(classes=2, blank=2), EINVAL, b'blank'),
        (dict(scores=P), EINVAL, b'both or neither'),
        (dict(starts=P), EINVAL, b'both or neither'),
        (dict(batch=-1), EINVAL, b'negative'),
        (dict(frames=-1), EINVAL, b'negative'),
    ]:
        rc, message = call(**change)
        assert rc == code and text in message, (change, rc, message)
    # nothing to do is not an error, and is decided on the host too: an empty batch; no frames with the state committed in place
    assert call(batch=0)[0] == 0
    assert call(frames=0, x=None)[0] == 0
    assert call(batch=0, x=None, frames=7, scores=P, starts=P)[0] == 0


# ---- the session's signature ---------------------------------------------------------------------------------------------------------
def test_session_signature():
    params = inspect.signature(streaming.StreamingSession.__init__).parameters
    names = list(params)
    assert params['keywords'].kind is inspect.Parameter.KEYWORD_ONLY and params['keywords'].default is None
    assert names.index('endpoint') < names.index('keywords') < names.index('lm') and names[-3:] == ['lm', 'alpha', 'beta']
    assert 'keywords' not in inspect.signature(model_module.ASRModel.stream).parameters         # stream() keeps its parameter list
    assert isinstance(streaming.StreamingSession.keywords, property) and callable(streaming.StreamingSession.peek_keywords)
    assert 'provisional' in streaming.StreamingSession.peek_keywords.__doc__.lower()
