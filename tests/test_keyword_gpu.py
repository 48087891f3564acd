"""The keyword spotter on the device: the kernel against the definition (keyword_model.py) bit for bit on every state word and both
traces, results that depend neither on the chunking, nor on the batch, nor on the other keywords of the set, a peek that changes nothing,
and streaming sessions made with ``keywords=``.

Values: a grid of 0.25 (exact ties between candidates and between frames are frequent) and model-scale random float32 logits.  Denormal
values are NOT exercised: no case here produces a float32 below 2^-126 in magnitude other than 0, so the denormal mode of the device
and of numpy is never compared."""
import functools
import json

import numpy as np
import pytest
import torch

import cases
import keyword_model as km
import test_stream_launch_sequence_gpu as tsl
from nb_asr_amd import ctc, frontend, hip, streaming
from test_launch_sequence_gpu import summarise
from test_stream_launch_sequence_gpu import features, model_for, waves

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
BATCH = 5
FRAMES = (0, 1, 63, 64, 65, 128, 200)
CLASSES = (2, 33, 49, 65, 128)
BLANK = 0


def lengths_for(n):
    return (n, 0, n // 2, max(n - 1, 0), n)                       # the full length, nothing (a row of length 0), and in between


def collapse(labels):
    out, prev = [], None
    for v in labels:
        if v != prev and v != BLANK:
            out.append(int(v))
        prev = v
    return out


@functools.lru_cache(maxsize=None)
def case(n, classes, kind='grid'):
    """(x (5, n, C) on the device with NaN beyond each row's length, the same on the host, lengths)."""
    rng = np.random.default_rng(1000 * classes + n + (0 if kind == 'grid' else 7))
    if kind == 'grid':
        x = (rng.integers(-8, 9, size=(BATCH, n, classes)) / 4).astype(np.float32)
        x[:, :, BLANK] += (rng.integers(0, 3, size=(BATCH, n)) / 2).astype(np.float32)        # the blank wins many frames, and ties others
    else:
        x = (rng.standard_normal((BATCH, n, classes)) * 3).astype(np.float32)                 # model-scale logits
        x[:, :, BLANK] += (rng.random((BATCH, n)) < 0.5).astype(np.float32) * 4
    lengths = np.array(lengths_for(n), dtype=np.int32)
    for b in range(BATCH):
        x[b, lengths[b]:] = np.nan
    x.setflags(write=False)
    return torch.from_numpy(x.copy()).to(DEV), x, lengths


@functools.lru_cache(maxsize=None)
def keyword_mix(n, classes, kind='grid'):
    """Keywords of 1, 2, 31 and 32 tokens (S = 1 and S = 63: lanes 62 and 63 matter), a repeated-token one, 32 times the same token,
    two identical ones, and -- where the rows are long enough -- what row 0's greedy path spells over its first frames (score 0 there).
    Thresholds from 0 (only an exact match hits) to -1000 (the first frame with a path hits)."""
    rng = np.random.default_rng(77 * classes + n)
    tok = lambda count: tuple(int(v) for v in rng.integers(1, classes, size=count))
    a, b = tok(1)[0], tok(1)[0]
    words = [tok(1), tok(2), tok(31), tok(32), (a, a, b), (a,) * 32]
    words.append(words[1])                                                              # two identical keywords
    thresholds = [0.0, -1.0, -15.5, -1000.0, -2.25, -40.0, -3.0]
    _, x, lengths = case(n, classes, kind)
    spelled = collapse(x[0, :min(n, 50)].argmax(1).tolist()) if n else []
    if len(spelled) >= 2:
        words += [tuple(spelled[:32]), tuple(spelled[:2])]
        thresholds += [0.0, 0.0]
    return tuple(words), tuple(thresholds)


@functools.lru_cache(maxsize=None)
def model_whole(n, classes, kind='grid'):
    words, thresholds = keyword_mix(n, classes, kind)
    _, x, lengths = case(n, classes, kind)
    out = km.step(x, lengths, None, words, thresholds, BLANK)
    for a in out:
        a.setflags(write=False)
    return out


def bits(t):
    """A device or host tensor / array as int32 words on the host: float32 values compare by their bits."""
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return a.view(np.int32) if a.dtype == np.float32 else a


def host(result):
    """(B, K, 136) int32 on the host, checked against the named fields."""
    state = result.state.cpu().numpy()
    for name, want in km.fields(state).items():
        got = getattr(result, name)
        assert got.shape == state.shape[:2] and got.dtype == (torch.float32 if 'score' in name else torch.int32), name
        assert np.array_equal(bits(got), bits(want)), name
    assert np.array_equal(result.detected.cpu().numpy(), state[:, :, 1] >= 0)
    return state


def check_whole(n, classes, kind='grid'):
    x, _, lengths = case(n, classes, kind)
    words, thresholds = keyword_mix(n, classes, kind)
    ks = ctc.KeywordSet(words, thresholds, classes=classes, blank=BLANK, device=DEV)
    want, want_scores, want_starts = model_whole(n, classes, kind)
    result, scores, starts = ctc.spot_keywords(x, lengths, ks, return_trace=True)
    assert scores.shape == starts.shape == (BATCH, len(words), n) and scores.dtype == torch.float32 and starts.dtype == torch.int32
    state = host(result)
    assert np.array_equal(state, want), (n, classes, kind, np.argwhere(state != want)[:8])
    assert np.array_equal(bits(scores), bits(want_scores)) and np.array_equal(bits(starts), want_starts), (n, classes, kind)
    assert np.array_equal(host(ctc.spot_keywords(x, lengths, ks)), want)               # (without the trace)
    return km.fields(want), want_scores


@pytest.mark.parametrize('kind', ('grid', 'random'))
@pytest.mark.parametrize('n', FRAMES)
def test_kernel_equals_model_at_every_length(n, kind):
    f, scores = check_whole(n, 49, kind)
    assert np.array_equal(f['frames'], np.repeat(np.array(lengths_for(n))[:, None], f['frames'].shape[1], 1))
    assert (f['hit_frame'][1] == -1).all() and np.isneginf(f['best_score'][1]).all()   # the row of length 0 stays fresh
    if n >= 65:
        words, _ = keyword_mix(n, 49, kind)
        assert len(words) == 9                                                          # the greedy path's keywords are there ...
        assert f['hit_score'][0, 7] == 0 and f['hit_score'][0, 8] == 0                  # ... and are found with score 0 (threshold 0)
        for k in (3, 5):                                                                # 32 tokens: a path needs a frame per token and a blank
            need = len(words[k]) + sum(p == q for p, q in zip(words[k], words[k][1:]))  # between equal neighbours (32 times one token: 63 frames)
            assert np.isneginf(scores[0, k, :need - 1]).all() and np.isfinite(scores[0, k, need - 1]), k


@pytest.mark.parametrize('kind', ('grid', 'random'))
@pytest.mark.parametrize('classes', CLASSES)
def test_kernel_equals_model_at_every_class_count(classes, kind):
    check_whole(129, classes, kind)


@functools.lru_cache(maxsize=None)
def many_keywords(count, classes=49):
    rng = np.random.default_rng(count)
    words = [tuple(int(v) for v in rng.integers(1, classes, size=int(rng.integers(1, 33)))) for _ in range(count)]
    words[0] = (3, 4)
    if count > 2:
        words[1], words[2] = (6, 6, 2), (3, 4)                                         # a repeated token; identical to keyword 0
    if count > 3:
        words[-1] = (9,) * 32                                                           # S = 63 without a skip
    thresholds = [-(k % 7) * 1.25 for k in range(count)]
    if count > 2:
        thresholds[2] = thresholds[0]
    return tuple(words), tuple(thresholds)


@functools.lru_cache(maxsize=None)
def model_many(count, n):
    words, thresholds = many_keywords(count)
    _, x, _ = case(n, 49)
    return km.step(x[[0, 4]], np.array([n, n // 3], dtype=np.int32), None, words, thresholds, BLANK)       # rows 0 and 4 are full rows


@pytest.mark.parametrize('count', (1, 3, 8, 9, 64))
def test_kernel_equals_model_at_every_keyword_count(count):
    """1, 3 and 64 keywords; 8 and 9 are one full workgroup of waves and one wave more."""
    n = 130
    x, _, _ = case(n, 49)
    rows = np.array([n, n // 3], dtype=np.int32)
    words, thresholds = many_keywords(count)
    ks = ctc.KeywordSet(words, thresholds, device=DEV)
    want, want_scores, want_starts = model_many(count, n)
    result, scores, starts = ctc.spot_keywords(x[[0, 4]].contiguous(), rows, ks, return_trace=True)
    assert np.array_equal(host(result), want)
    assert np.array_equal(bits(scores), bits(want_scores)) and np.array_equal(bits(starts), want_starts)
    if count > 2:
        assert np.array_equal(want[:, 0], want[:, 2])                                    # two identical keywords: identical rows


def test_a_keyword_alone_equals_the_same_keyword_among_64():
    x, _, lengths = case(130, 49)
    words, thresholds = many_keywords(64)
    full = ctc.spot_keywords(x, lengths, ctc.KeywordSet(words, thresholds, device=DEV), return_trace=True)
    for k in (0, 1, 7, 8, 31, 63):
        alone = ctc.spot_keywords(x, lengths, ctc.KeywordSet([words[k]], [thresholds[k]], device=DEV), return_trace=True)
        assert torch.equal(alone[0].state[:, 0], full[0].state[:, k]), k
        assert np.array_equal(bits(alone[1][:, 0]), bits(full[1][:, k])) and torch.equal(alone[2][:, 0], full[2][:, k]), k


def test_rows_beyond_their_length_are_not_read_and_lengths_are_optional():
    x, _, lengths = case(129, 49)
    words, thresholds = keyword_mix(129, 49)
    ks = ctc.KeywordSet(words, thresholds, device=DEV)
    clean = torch.nan_to_num(x, nan=3.0)
    a, b = ctc.spot_keywords(x, lengths, ks, return_trace=True), ctc.spot_keywords(clean, lengths, ks, return_trace=True)
    assert torch.equal(a[0].state, b[0].state) and np.array_equal(bits(a[1]), bits(b[1])) and torch.equal(a[2], b[2])
    assert not torch.isnan(a[1]).any()
    whole, scores, starts = ctc.spot_keywords(clean[:2].contiguous(), None, ks, return_trace=True)
    want, want_scores, want_starts = km.step(clean[:2].cpu().numpy(), None, None, words, thresholds, BLANK)
    assert np.array_equal(host(whole), want) and np.array_equal(bits(scores), bits(want_scores)) and np.array_equal(bits(starts), want_starts)
    assert (want[:, :, 0] == 129).all()


def test_nan_inside_a_row_is_the_models_nan():
    """A NaN that is read: in a keyword's class, and a whole frame of them.  The words are the model's; where both hold a NaN the
    payloads may differ (the device and the host choose their own), so those words compare as NaN = NaN."""
    _, xh, _ = case(65, 33, 'random')
    x = xh[:1].copy()
    words = ((4, 7), (9,), (7, 7, 4))
    x[0, 20, 7] = np.nan
    x[0, 40, :] = np.nan
    x[0, 64, 9] = np.nan                                                                # the last frame: the NaN is in the state that is left
    thresholds = (-3.0, -0.5, -6.0)
    want, want_scores, want_starts = km.step(x, None, None, words, thresholds, BLANK)
    result, scores, starts = ctc.spot_keywords(torch.from_numpy(x).to(DEV), None, ctc.KeywordSet(words, thresholds, classes=33, device=DEV), return_trace=True)
    assert np.isnan(want_scores[0, :, 40]).all() and np.isnan(want_scores[0, 1, 64]) and np.isnan(want[0, 1, 8:9].view(np.float32))[0]
    assert np.array_equal(scores.cpu().numpy(), want_scores, equal_nan=True) and np.array_equal(bits(starts), want_starts)
    state = host(result)
    assert np.array_equal(state[:, :, :8], want[:, :, :8]) and np.array_equal(state[:, :, 72:], want[:, :, 72:])
    assert np.array_equal(state[:, :, 8:72].view(np.float32), want[:, :, 8:72].view(np.float32), equal_nan=True)


# ---- planted keywords ----------------------------------------------------------------------------------------------------------------
WORD, SHORT = (7, 9, 7), (5,)
PLANT_FRAMES = 130
PLANTS = {'ending at frame 63': 60, 'ending at frame 64': 61, 'across the pass boundary': 62, 'across the chunk boundary': 98, 'never': None}


@functools.lru_cache(maxsize=None)
def planted():
    """Row i holds plant i of WORD as the strict per-frame maxima 7 7 9 7 from its start (the hit is the first frame of the last token,
    start + 3), everything else won by the blank; row 0 also starts with SHORT at frame 0.  Noise on a grid of 0.25 below the maxima."""
    rng = np.random.default_rng(11)
    x = (rng.integers(-8, 1, size=(len(PLANTS), PLANT_FRAMES, 49)) / 4).astype(np.float32)
    x[:, :, BLANK] = 1.0
    for row, at in enumerate(PLANTS.values()):
        if at is not None:
            for t, label in zip(range(at, at + 4), (7, 7, 9, 7)):
                x[row, t, BLANK], x[row, t, label] = 0.0, 1.0
    x[0, 0, BLANK], x[0, 0, SHORT[0]] = 0.0, 1.0
    return torch.from_numpy(x).to(DEV), x


def test_planted_keywords_are_found_where_they_are():
    x, xh = planted()
    ks = ctc.KeywordSet([WORD, SHORT], thresholds=0.0, device=DEV)                      # only an exact match hits
    want = km.step(xh, None, None, [WORD, SHORT], [0.0, 0.0], BLANK)[0]
    whole = host(ctc.spot_keywords(x, None, ks))
    stream = ctc.KeywordStream(len(PLANTS), ks, DEV)
    for chunk in (x[:, :100], x[:, 100:]):                                              # the chunk boundary: frames 98 99 | 100 101
        chunked = host(stream.push(chunk))
    assert np.array_equal(whole, want) and np.array_equal(chunked, want)
    f = km.fields(whole)
    for row, at in enumerate(PLANTS.values()):
        if at is None:
            assert f['hit_frame'][row, 0] == -1 and f['hit_start'][row, 0] == -1 and f['best_score'][row, 0] < 0
        else:
            assert (f['hit_frame'][row, 0], f['hit_start'][row, 0], f['hit_score'][row, 0]) == (at + 3, at, 0.0), row
            assert (f['best_frame'][row, 0], f['best_start'][row, 0], f['best_score'][row, 0]) == (at + 3, at, 0.0), row
    assert (f['hit_frame'][0, 1], f['hit_start'][0, 1], f['hit_score'][0, 1]) == (0, 0, 0.0)               # ending at frame 0
    assert (f['hit_frame'][1:, 1] == -1).all()
    assert [PLANTS[k] + 3 for k in list(PLANTS)[:2]] == [63, 64]


# ---- chunking, batching, peek --------------------------------------------------------------------------------------------------------
CUTS = (1, 7, 63, 64, 65, 200)
SIZES = (1, 0, 6, 0, 56, 1, 0, 1, 0, 135)                        # cuts at 1, 7, 63, 64 and 65, with empty pushes in between


def chunks(x, lengths):
    """[(chunk, its lengths)] of x cut into SIZES."""
    at, out = 0, []
    for k in SIZES:
        out.append((x[:, at:at + k], np.clip(lengths - at, 0, k)))
        at += k
    assert at == x.shape[1] and sorted(set(np.cumsum(SIZES).tolist())) == list(CUTS)
    return out


@pytest.mark.parametrize('kind', ('grid', 'random'))
def test_chunked_equals_whole_equals_a_row_alone(kind):
    x, xh, lengths = case(200, 49, kind)
    words, thresholds = keyword_mix(200, 49, kind)
    ks = ctc.KeywordSet(words, thresholds, device=DEV)
    want, want_scores, _ = model_whole(200, 49, kind)
    whole = host(ctc.spot_keywords(x, lengths, ks))
    assert np.array_equal(whole, want)
    stream = ctc.KeywordStream(BATCH, ks, DEV)
    for repeat in range(2):                                        # the second time after reset(), over a used state
        assert np.array_equal(host(stream.result), km.fresh(BATCH, len(words)))
        state = None
        for chunk, rows in chunks(x, lengths):
            got = host(stream.push(chunk, rows))
            if chunk.shape[1] in (6, 56):                          # the model chunk by chunk too, at two of the cuts
                state = km.step(xh[:, :int(got[0, 0, 0])], np.minimum(lengths, got[0, 0, 0]), None, words, thresholds, BLANK)[0]
                assert np.array_equal(got, state)
            assert np.array_equal(got, host(stream.result))
        assert np.array_equal(got, whole)
        stream.reset()
    for b in range(BATCH):
        alone = ctc.KeywordStream(1, ks, DEV)
        for chunk, rows in chunks(x, lengths):
            got = host(alone.push(chunk[b:b + 1].contiguous(), rows[b:b + 1]))
        assert np.array_equal(got, whole[b:b + 1])
        assert np.array_equal(host(ctc.spot_keywords(x[b:b + 1], lengths[b:b + 1], ks)), whole[b:b + 1])
    full = ctc.KeywordStream(BATCH, ks, DEV)                      # without lengths: every row takes every frame
    clean = torch.nan_to_num(x, nan=-1.0)
    for chunk, _ in chunks(clean, lengths):
        got = host(full.push(chunk))
    assert np.array_equal(got, host(ctc.spot_keywords(clean, None, ks)))


def test_peek_equals_a_twins_push_and_changes_nothing():
    x, _, lengths = case(200, 49)
    words, thresholds = keyword_mix(200, 49)
    ks = ctc.KeywordSet(words, thresholds, device=DEV)
    stream, twin = ctc.KeywordStream(BATCH, ks, DEV), ctc.KeywordStream(BATCH, ks, DEV)
    size = stream.state_bytes
    assert size == 2 * hip.ctc_keyword_state_bytes(BATCH, len(words))                   # the committed record and the constant fresh one
    assert np.array_equal(host(stream.peek()), km.fresh(BATCH, len(words)))             # before any frame
    for chunk, rows in chunks(x, lengths):
        before = stream.state.clone()
        peeked = host(stream.peek(chunk, rows))
        assert torch.equal(stream.state, before)                   # the committed record is only read
        assert np.array_equal(host(stream.peek()), host(stream.result))
        pushed = host(twin.push(chunk, rows))
        assert np.array_equal(peeked, pushed)
        assert np.array_equal(host(stream.peek(chunk, rows)), pushed)                   # a second peek: the same
        assert np.array_equal(host(stream.push(chunk, rows)), pushed)                   # every later result: a stream that never peeked
    assert stream.state_bytes == size + hip.ctc_keyword_state_bytes(BATCH, len(words))  # the peek record, made by the first peek


def test_stream_contract_and_refusals():
    ks = ctc.KeywordSet([(3, 4), (5,)], device=DEV)
    stream = ctc.KeywordStream(2, ks, DEV)
    good = torch.zeros(2, 3, 49, device=DEV)
    entries = []
    hip.start_tape(entries)
    try:
        stream.reset()
        stream.push(good[:, :0])
        stream.peek(good[:, :0])
        stream.peek()
        assert entries == [] and stream._peek_state is None       # reset, pushes and peeks of no frames: no launch, no peek record
        stream.push(good)
        stream.peek(good)
    finally:
        hip.stop_tape()
    assert [fn.__name__ for fn, _ in entries] == ['nbasr_ctc_keyword_step'] * 2 and stream._peek_state is not None
    stream.reset()
    for bad, match in ((good[:1], 'expected'), (good[:, :, :48], 'classes'), (good.double(), 'float32'), (good.cpu(), 'HIP device')):
        with pytest.raises(ValueError, match=match):
            stream.push(bad)
        with pytest.raises(ValueError, match=match):
            stream.peek(bad)
    for lengths in ((1,), (1, 4), (-1, 0)):
        with pytest.raises(ValueError, match='lengths'):
            stream.push(good, lengths)
    stream.push(good, (3, 2))
    with pytest.raises(ValueError, match='has ended'):
        stream.push(good, (1, 1))
    assert host(stream.push(good, (3, 0)))[:, :, 0].tolist() == [[6, 6], [2, 2]]
    tokens, counts, thresholds = ks.tables
    with pytest.raises(hip.HipError, match='both or neither'):
        hip.ctc_keyword_step(good, None, tokens, counts, thresholds, 0, None, stream.state, torch.zeros(2, 2, 3, device=DEV))
    with pytest.raises(hip.HipError, match='blank'):
        hip.ctc_keyword_step(good, None, tokens, counts, thresholds, 49, None, stream.state)
    empty = torch.zeros(0, 3, 49, device=DEV)                      # an empty batch: nothing to do
    assert ctc.spot_keywords(empty, None, ks).state.shape == (0, 2, 136)
    hit_start, hit_end, best_start, best_end = stream.result.seconds()
    assert hit_start.shape == (2, 2) and hit_start.dtype == torch.float32 and best_end.is_cuda
    kept = stream.result.clone()
    stream.reset()
    assert kept.frames.tolist() == [[6, 6], [2, 2]] and stream.result.frames.tolist() == [[0, 0], [0, 0]]


# ---- sessions --------------------------------------------------------------------------------------------------------------------------
def feed(sess, piece, audio, decode):
    return sess.push_audio(piece, decode=decode) if audio else sess.push(piece, decode=decode)


def same(a, b):
    """Bit for bit, through the tuples and lists a push / flush / peek returns."""
    if isinstance(a, torch.Tensor):
        return isinstance(b, torch.Tensor) and a.shape == b.shape and torch.equal(a, b)
    return type(a) is type(b) and len(a) == len(b) and all(same(p, q) for p, q in zip(a, b))


def logits_of(out):
    return out if isinstance(out, torch.Tensor) else out[0]


def keyword_calls(entries):
    return [fn.__name__ for fn, _ in entries].count('nbasr_ctc_keyword_step')


@pytest.mark.parametrize('audio,decode', [(False, True), (True, False), (False, 'beam')])
def test_sessions(audio, decode):
    model = model_for(cases.ARCH_M, True)
    if audio:
        x, sizes = waves(2, 48000, 60), (16000, 16000, 0, 12000, 4000)
        make = lambda **kw: streaming.StreamingSession(model, 2, max_chunk=64, frontend=frontend.LogMelFrontend(device=DEV), **kw)
    else:
        x, sizes = features(2, 400, 6), (100, 150, 0, 90, 60)
        make = lambda **kw: streaming.StreamingSession(model, 2, max_chunk=64, beam_width=4, **kw)
    with torch.no_grad():
        plain = make()
        assert plain.keywords is None
        with pytest.raises(ValueError, match='keyword'):
            plain.peek_keywords()
        # the plain session first: its logits choose the keywords, and it is what a session with keywords= must return
        at, plain_outs, plain_peeks = 0, [], []
        for n in sizes:
            plain_outs.append(feed(plain, x[..., at:at + n], audio, decode))
            plain_peeks.append(plain.peek(decode))
            at += n
        plain_outs.append(plain.flush(decode))
        parts = [logits_of(o) for o in plain_outs]
        emitted = np.cumsum([p.shape[1] for p in parts])
        total = int(emitted[-1])
        whole = torch.cat(parts, 1).contiguous()
        assert emitted[0] == 0 and 0 < emitted[len(sizes) - 1] < total, emitted   # a push that emits nothing, frames before the flush
        # keywords from the model's own logits: what row 0's greedy path spells (score 0 where it does), and two it may never say
        spelled = collapse(whole[0].argmax(1).tolist())
        words = ([tuple(spelled[:3])] if spelled else []) + [(3, 4), (20, 20, 21)]
        thresholds = [0.0] * (len(words) - 2) + [-2.0, -30.0]
        ks = ctc.KeywordSet(words, thresholds, device=DEV)
        wh = whole.cpu().numpy()
        want_whole = km.step(wh, None, None, words, thresholds, BLANK)[0]
        if spelled:
            assert (want_whole[0, 0, 1] >= 0) and want_whole[0, 0, 3:4].view(np.float32)[0] == 0

        sess = make(keywords=ks)
        state_bytes = 2 * hip.ctc_keyword_state_bytes(2, len(words))
        assert sess.buffer_bytes - make().buffer_bytes == sess._keywords.state_bytes == state_bytes
        for repeat in range(2):                                    # the second time after reset()
            assert np.array_equal(host(sess.keywords), km.fresh(2, len(words)))
            at = 0
            for i, n in enumerate(sizes):
                piece = x[..., at:at + n]
                entries = []
                hip.start_tape(entries)
                try:
                    out = feed(sess, piece, audio, decode)
                finally:
                    hip.stop_tape()
                assert same(out, plain_outs[i])                    # exactly what a session without keywords= returns
                at, done = at + n, int(emitted[i])
                assert keyword_calls(entries) == (1 if parts[i].shape[1] else 0)         # one more launch when frames were emitted
                if parts[i].shape[1]:
                    assert entries[-1][0].__name__ == 'nbasr_ctc_keyword_step'          # after the decode launches
                committed = host(sess.keywords)
                assert np.array_equal(committed, km.step(wh[:, :done], None, None, words, thresholds, BLANK)[0])
                if done:
                    assert np.array_equal(committed, host(ctc.spot_keywords(whole[:, :done].contiguous(), None, ks)))
                entries = []
                hip.start_tape(entries)
                try:
                    peeked, ahead = sess.peek_keywords(decode)
                finally:
                    hip.stop_tape()
                assert same(peeked, plain_peeks[i])                # peek's own result, bit for bit
                assert keyword_calls(entries) == (1 if logits_of(peeked).shape[1] else 0)
                both = torch.cat([whole[:, :done], logits_of(peeked)], 1).contiguous()
                assert np.array_equal(host(ahead), km.step(both.cpu().numpy(), None, None, words, thresholds, BLANK)[0])
                assert np.array_equal(host(sess.keywords), committed)                   # the peek left the committed result alone
                if repeat == 0 and i in (1, len(sizes) - 1):       # a twin that is flushed here: what the peek showed
                    twin, t_at = make(keywords=ks), 0
                    for m in sizes[:i + 1]:
                        feed(twin, x[..., t_at:t_at + m], audio, decode)
                        t_at += m
                    twin.flush(decode)
                    assert np.array_equal(host(twin.keywords), host(ahead))
            entries = []
            hip.start_tape(entries)
            try:
                out = sess.flush(decode)
            finally:
                hip.stop_tape()
            assert same(out, plain_outs[-1]) and keyword_calls(entries) == 1
            assert np.array_equal(host(sess.keywords), want_whole)
            assert np.array_equal(host(ctc.spot_keywords(whole, None, ks)), want_whole)
            sess.reset()
            assert np.array_equal(host(sess.keywords), km.fresh(2, len(words)))         # reset() clears the result
        assert sess._keywords.state_bytes == 3 * hip.ctc_keyword_state_bytes(2, len(words))              # the peek record, counted in
        assert sess.buffer_bytes - make().buffer_bytes > sess._keywords.state_bytes                       # buffer_bytes with the session's own


def run_greedy_scenario(**kw):
    """The 'greedy' scenario of test_stream_launch_sequence_gpu.py, its session made with ``kw``: the tape of the recorded pass."""
    sess = streaming.StreamingSession(model_for(cases.ARCH_M, True), 2, max_chunk=64, **kw)
    x = features(2, 280, 1)

    def script():
        sess.peek(True)
        tsl.pushes(sess, x, (100, 150, 0, 30), True)
    with torch.no_grad():
        script()
        sess.reset()
        entries = []
        hip.start_tape(entries)
        try:
            script()
        finally:
            hip.stop_tape()
    torch.cuda.synchronize()
    return sess, entries


def test_a_session_without_keywords_is_the_recorded_one_launch_for_launch():
    """The route recorded before the spotter existed (tests/golden/stream_launch_sequences.json): a session without ``keywords=``
    makes exactly those calls; one with it makes them too, with nothing but its own step added."""
    want = json.loads(tsl.FIXTURE.read_text())['greedy']
    assert summarise(tsl.record('greedy')) == want                 # the recorder's own scenario: model.stream(...)
    sess, entries = run_greedy_scenario()
    assert keyword_calls(entries) == 0 and summarise(tsl.normalise(sess, entries)) == want
    sess, entries = run_greedy_scenario(keywords=ctc.KeywordSet([(3, 4), (5,)], device=DEV))
    others = [e for e in entries if e[0].__name__ != 'nbasr_ctc_keyword_step']
    assert 0 < keyword_calls(entries) <= 4 and len(others) == len(want['names'])
    assert summarise(tsl.normalise(sess, others)) == want


def test_session_refusals():
    model = model_for(cases.ARCH_M, True)
    with pytest.raises(ValueError, match='KeywordSet'):
        streaming.StreamingSession(model, 1, keywords=[[3, 4]])
    with pytest.raises(ValueError, match='classes'):
        streaming.StreamingSession(model, 1, keywords=ctc.KeywordSet([[3, 4]], classes=48))
    both = streaming.StreamingSession(model, 1, endpoint=ctc.EndpointRules(device=DEV), keywords=ctc.KeywordSet([[3, 4]], device=DEV))
    assert both.endpoint is not None and both.keywords is not None
