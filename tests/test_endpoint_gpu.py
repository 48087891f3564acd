"""The endpointer on the device: the kernel against the definition (endpoint_model.py) bit for bit on every output, results that do not
depend on the chunking or the batch, a peek that changes nothing, and streaming sessions made with ``endpoint=``."""
import functools

import numpy as np
import pytest
import torch

import cases
import endpoint_model as em
from nb_asr_amd import ctc, frontend, hip, streaming
from test_stream_launch_sequence_gpu import features, model_for, waves

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
BATCH = 5
FRAMES = (0, 1, 63, 64, 65, 128, 129, 200)
CLASSES = (2, 33, 49, 64, 65, 128)
# (name, rules): where the endpoint falls for a row of at least that many frames
RULE_SETS = (
    ('at frame 0', ((0, 0, 0),)),
    ('at frame 63, a pass\'s last', ((0, 0, 64),)),
    ('at frame 64, a pass\'s first', ((0, 0, 65),)),
    ('in the middle of a later pass', ((0, 0, 100),)),
    ('never', ((10 ** 6, 0, 0), (0, 10 ** 6, 0))),
    ('two rules at the same frame', ((10 ** 6, 0, 0), (0, 0, 64), (0, 0, 64))),
    ('two rules at the same frame, later', ((0, 0, 130), (0, 0, 130))),
    ('by what was said', ((3, 2, 0), (0, 7, 0), (20, 0, 0), (0, 0, 150))),
    ('eight rules', ((50, 3, 0), (40, 2, 70), (1, 9, 0), (0, 12, 0), (0, 0, 190), (2, 1, 66), (7, 0, 128), (0, 64, 0))),
)


def speech_set(classes):
    """Two classes: class 1.  Otherwise the classes that are no multiple of 3 -- from 65 classes on that has bits in both mask words."""
    return (1,) if classes == 2 else tuple(c for c in range(1, classes) if c % 3)


def lengths_for(n):
    return (n, 0, n // 2, max(n - 1, 0), n)                       # the full length, nothing, and in between


@functools.lru_cache(maxsize=None)
def case(n, classes):
    """(x (5, n, C) on the device with NaN beyond each row's length, the same on the host, lengths): values on a grid of 0.25 so that
    the two maxima tie exactly in many frames (and differ by exactly 0.5 in others); row 3 is all speech, row 4 has none."""
    rng = np.random.default_rng(1000 * classes + n)
    x = (rng.integers(-8, 9, size=(BATCH, n, classes)) / 4).astype(np.float32)
    speech = speech_set(classes)
    quiet = [c for c in range(classes) if c not in speech]
    x[:, :, quiet] -= (rng.integers(0, 4, size=(BATCH, n, 1)) / 4).astype(np.float32)       # the gap between the maxima: a few steps either way
    x[3][:, speech[-1]] = 5.0
    x[4][:, quiet[-1]] = 5.0
    lengths = np.array(lengths_for(n), dtype=np.int32)
    for b in range(BATCH):
        x[b, lengths[b]:] = np.nan
    x.setflags(write=False)
    return torch.from_numpy(x.copy()).to(DEV), x, lengths


@functools.lru_cache(maxsize=None)
def model_mask(n, classes, margin):
    _, x, lengths = case(n, classes)
    mask = em.speech_mask(x, lengths, speech_set(classes), margin)
    mask.setflags(write=False)
    return mask


def host(result):
    """(B, 8) int32 on the host, checked against the named fields."""
    state = result.state.cpu().numpy()
    for k, name in enumerate(ctc.EndpointResult.FIELDS):
        assert np.array_equal(getattr(result, name).cpu().numpy(), state[:, k]), name
        assert getattr(result, name).dtype == torch.int32 and getattr(result, name).shape == (state.shape[0],)
    return state


def check_whole(n, classes, margin):
    x, _, lengths = case(n, classes)
    want_mask = model_mask(n, classes, margin)
    for name, rules in RULE_SETS:
        r = ctc.EndpointRules(rules, speech_set(classes), margin, classes, DEV)
        result, mask = ctc.endpoint(x, lengths, r, return_mask=True)
        want = em.scan(want_mask, lengths, None, rules)
        assert np.array_equal(mask.cpu().numpy(), want_mask), (n, classes, margin, name)
        assert np.array_equal(host(result), want), (n, classes, margin, name, host(result), want)
        assert np.array_equal(host(ctc.endpoint(x, lengths, r)), want)                 # (without the mask)
    return want_mask


@pytest.mark.parametrize('margin', (0.0, 0.5))
@pytest.mark.parametrize('n', FRAMES)
def test_kernel_equals_model_at_every_length(n, margin):
    mask = check_whole(n, 49, margin)
    lengths = lengths_for(n)
    assert mask[3].sum() == lengths[3] and mask[4].sum() == 0                          # all speech, no speech
    if n >= 63 and margin == 0.0:
        assert 0 < mask[0].sum() < n


@pytest.mark.parametrize('margin', (0.0, 0.5))
@pytest.mark.parametrize('classes', CLASSES)
def test_kernel_equals_model_at_every_class_count(classes, margin):
    check_whole(129, classes, margin)
    speech = speech_set(classes)
    if classes > 64:
        assert min(speech) < 64 <= max(speech)                                          # bits in both words of the mask


def test_the_cases_hold_what_they_are_for():
    """Exact ties of the two maxima (non-speech at margin 0), gaps of exactly the margin (non-speech at 0.5), and each rule set's place."""
    _, x, lengths = case(200, 49)
    speech = list(speech_set(49))
    quiet = [c for c in range(49) if c not in speech]
    ms, mn = x[0][:, speech].max(1), x[0][:, quiet].max(1)
    assert (ms == mn).sum() > 20 and (ms == mn + 0.5).sum() > 5 and (ms > mn + 0.5).sum() > 5
    assert not model_mask(200, 49, 0.0)[0][ms == mn].any() and not model_mask(200, 49, 0.5)[0][ms == mn + 0.5].any()
    assert model_mask(200, 49, 0.0)[0][ms == mn + 0.5].all()
    ends = {name: em.scan(model_mask(200, 49, 0.0), lengths, None, rules)[0, 4:6].tolist() for name, rules in RULE_SETS}
    assert ends['at frame 0'] == [0, 0] and ends['at frame 63, a pass\'s last'] == [63, 0] and ends['at frame 64, a pass\'s first'] == [64, 0]
    assert ends['in the middle of a later pass'] == [99, 0] and ends['never'] == [-1, -1]
    assert ends['two rules at the same frame'] == [63, 1] and ends['two rules at the same frame, later'] == [129, 0]
    assert ends['by what was said'][1] in (0, 1, 2) and ends['eight rules'][0] >= 0


def test_rows_beyond_their_length_are_not_read_and_lengths_are_optional():
    x, xh, lengths = case(129, 49)
    rules = ctc.EndpointRules(RULE_SETS[7][1], speech_set(49), 0.0, 49, DEV)
    clean = torch.nan_to_num(x, nan=3.0)
    a, b = ctc.endpoint(x, lengths, rules, return_mask=True), ctc.endpoint(clean, lengths, rules, return_mask=True)
    assert torch.equal(a[0].state, b[0].state) and torch.equal(a[1], b[1])
    whole, mask = ctc.endpoint(clean, None, rules, return_mask=True)
    want, want_mask = em.step(clean.cpu().numpy(), None, None, rules.rules, speech_set(49), 0.0)
    assert np.array_equal(host(whole), want) and np.array_equal(mask.cpu().numpy(), want_mask)
    assert np.array_equal(want[:, 0], [129] * BATCH)


def test_a_shift_of_a_frame_changes_nothing_on_the_device():
    """Shifts that are exact in float32 (multiples of 0.25 on a grid of 0.25) keep every bit."""
    x, _, lengths = case(200, 49)
    clean = torch.nan_to_num(x, nan=0.0)
    shift = torch.from_numpy(np.random.default_rng(5).integers(-40, 40, size=(BATCH, 200, 1)).astype(np.float32) / 4).to(DEV)
    for margin in (0.0, 0.5):
        rules = ctc.EndpointRules(RULE_SETS[7][1], speech_set(49), margin, 49, DEV)
        a, b = ctc.endpoint(clean, lengths, rules, return_mask=True), ctc.endpoint(clean + shift, lengths, rules, return_mask=True)
        assert torch.equal(a[0].state, b[0].state) and torch.equal(a[1], b[1])


# ---- chunking, batching, peek ------------------------------------------------------------------------------------------------------
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


@pytest.mark.parametrize('name,rule_set', [RULE_SETS[i] for i in (1, 2, 3, 7, 8)])
def test_chunked_equals_whole_equals_a_row_alone(name, rule_set):
    x, _, lengths = case(200, 49)
    rules = ctc.EndpointRules(rule_set, speech_set(49), 0.0, 49, DEV)
    whole = host(ctc.endpoint(x, lengths, rules))
    assert np.array_equal(whole, em.scan(model_mask(200, 49, 0.0), lengths, None, rule_set))
    stream = ctc.EndpointStream(BATCH, rules, DEV)
    for repeat in range(2):                                        # the second time after reset(), over a used state
        assert np.array_equal(host(stream.result), em.fresh(BATCH))
        at, mask = 0, model_mask(200, 49, 0.0)
        for (chunk, rows), k in zip(chunks(x, lengths), SIZES):
            got = host(stream.push(chunk, rows))
            at += k
            assert np.array_equal(got, em.scan(mask[:, :at], np.minimum(lengths, at), None, rule_set)), (name, at)
            assert np.array_equal(got, host(stream.result))
        assert np.array_equal(got, whole)
        stream.reset()
    for b in range(BATCH):
        alone = ctc.EndpointStream(1, rules, DEV)
        for chunk, rows in chunks(x, lengths):
            got = host(alone.push(chunk[b:b + 1].contiguous(), rows[b:b + 1]))
        assert np.array_equal(got, whole[b:b + 1]) and np.array_equal(host(ctc.endpoint(x[b:b + 1], lengths[b:b + 1], rules)), whole[b:b + 1])
    full = ctc.EndpointStream(BATCH, rules, DEV)                  # without lengths: every row takes every frame
    clean = torch.nan_to_num(x, nan=-1.0)
    for chunk, _ in chunks(clean, lengths):
        got = host(full.push(chunk))
    assert np.array_equal(got, host(ctc.endpoint(clean, None, rules)))


def test_peek_equals_a_twins_push_and_changes_nothing():
    x, _, lengths = case(200, 49)
    rules = ctc.EndpointRules(RULE_SETS[7][1], speech_set(49), 0.0, 49, DEV)
    stream, twin = ctc.EndpointStream(BATCH, rules, DEV), ctc.EndpointStream(BATCH, rules, DEV)
    size = stream.state_bytes
    assert size == 2 * hip.ctc_endpoint_state_bytes(BATCH)        # the committed record and the constant fresh one
    assert np.array_equal(host(stream.peek()), em.fresh(BATCH))   # before any frame
    for chunk, rows in chunks(x, lengths):
        before = stream.state.clone()
        peeked = host(stream.peek(chunk, rows))
        assert torch.equal(stream.state, before)                   # the committed record is only read
        assert np.array_equal(host(stream.peek()), host(stream.result))
        pushed = host(twin.push(chunk, rows))
        assert np.array_equal(peeked, pushed)
        assert np.array_equal(host(stream.peek(chunk, rows)), pushed)                   # a second peek: the same
        assert np.array_equal(host(stream.push(chunk, rows)), pushed)                   # every later result: a stream that never peeked
    assert stream.state_bytes == size + hip.ctc_endpoint_state_bytes(BATCH)             # the peek record, made by the first peek


def test_stream_refusals():
    rules = ctc.EndpointRules(((0, 1, 0),), speech_set(49), 0.0, 49, DEV)
    stream = ctc.EndpointStream(2, rules, DEV)
    good = torch.zeros(2, 3, 49, device=DEV)
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
    assert host(stream.push(good, (3, 0)))[:, 0].tolist() == [6, 2]
    with pytest.raises(hip.HipError, match='n_rules|rules'):
        hip.ctc_endpoint_step(good, None, None, stream.state, torch.zeros(9, 3, dtype=torch.int32, device=DEV), 2, 0, 0.0)


# ---- sessions ----------------------------------------------------------------------------------------------------------------------
def feed(sess, piece, audio, decode):
    return sess.push_audio(piece, decode=decode) if audio else sess.push(piece, decode=decode)


def same(a, b):
    """Bit for bit, through the tuples and lists a push / flush / peek returns."""
    if isinstance(a, torch.Tensor):
        return isinstance(b, torch.Tensor) and a.shape == b.shape and torch.equal(a, b)
    return type(a) is type(b) and len(a) == len(b) and all(same(p, q) for p, q in zip(a, b))


def logits_of(out):
    return out if isinstance(out, torch.Tensor) else out[0]


def endpoint_calls(entries):
    return [fn.__name__ for fn, _ in entries].count('nbasr_ctc_endpoint_step')


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
        assert plain.endpoint is None
        with pytest.raises(ValueError, match='endpoint'):
            plain.peek_endpoint()
        # the plain session first: its logits choose the rules, and it is what a session with endpoint= must return
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
        # rules from the model's own logits: row 0 ends half way through the frames committed by the first push that commits any
        speech = ctc.default_speech_classes()
        mask = em.speech_mask(whole.cpu().numpy(), None, speech, 0.0)
        first = int(np.argmax(emitted > 0))
        assert first < len(sizes) - 1 and emitted[0] == 0, emitted    # a push that emits nothing, pushes after the endpoint
        target = int(emitted[first]) // 2
        said = int(mask[0, :target + 1].sum())
        rule_set = (((said, 0, 0),) if said else ()) + ((0, 0, target + 1),)
        rules = ctc.EndpointRules(rule_set, device=DEV)
        want_whole = em.scan(mask, None, None, rule_set)
        assert 0 <= want_whole[0, 4] <= target < total - 1

        sess, never = make(endpoint=rules), make(endpoint=rules)
        assert sess.buffer_bytes - make().buffer_bytes == sess._endpoint.state_bytes == 2 * hip.ctc_endpoint_state_bytes(2)
        for repeat in range(2):                                    # the second time after reset()
            assert np.array_equal(host(sess.endpoint), em.fresh(2))
            at, done, latched, latched_at = 0, 0, None, None
            for i, n in enumerate(sizes):
                piece = x[..., at:at + n]
                entries = []
                hip.start_tape(entries)
                try:
                    out = feed(sess, piece, audio, decode)
                finally:
                    hip.stop_tape()
                assert same(out, plain_outs[i])                    # exactly what a session without endpoint= returns
                assert same(feed(never, piece, audio, decode), out)
                at, done = at + n, int(emitted[i])
                assert endpoint_calls(entries) == (1 if parts[i].shape[1] else 0)        # one more launch when frames were emitted
                committed = host(sess.endpoint)
                assert np.array_equal(committed, em.scan(mask[:, :done], None, None, rule_set))
                assert np.array_equal(committed, host(never.endpoint))
                if done:
                    assert np.array_equal(committed, host(ctc.endpoint(whole[:, :done].contiguous(), None, rules)))
                if latched is not None:
                    assert np.array_equal(committed[:, 4:6], latched)                   # a committed endpoint stays put
                if latched is None and (committed[:, 4] >= 0).all():
                    latched, latched_at = committed[:, 4:6].copy(), i
                peeked, ahead = sess.peek_endpoint(decode)
                assert same(peeked, plain_peeks[i])                # peek's own result, bit for bit
                both = torch.cat([whole[:, :done], logits_of(peeked)], 1).contiguous()
                want = em.step(both.cpu().numpy(), None, None, rule_set, speech, 0.0)[0]
                assert np.array_equal(host(ahead), want)
                if both.shape[1]:
                    assert np.array_equal(want, host(ctc.endpoint(both, None, rules)))
                assert np.array_equal(host(sess.endpoint), committed)                   # the peek left the committed result alone
            assert latched_at == first < len(sizes) - 1                                 # the endpoint was committed mid-stream
            out = sess.flush(decode)
            assert same(out, plain_outs[-1]) and same(never.flush(decode), out)
            assert np.array_equal(host(sess.endpoint), want_whole) and np.array_equal(host(never.endpoint), want_whole)
            assert np.array_equal(host(ctc.endpoint(whole, None, rules)), want_whole)
            assert np.array_equal(want_whole[:, 4:6], latched)
            sess.reset()
            never.reset()
        assert sess.buffer_bytes > never.buffer_bytes                                    # the peek's records, the endpointer's among them


def test_session_refusals():
    model = model_for(cases.ARCH_M, True)
    with pytest.raises(ValueError, match='EndpointRules'):
        streaming.StreamingSession(model, 1, endpoint=((0, 1, 0),))
    with pytest.raises(ValueError, match='classes'):
        streaming.StreamingSession(model, 1, endpoint=ctc.EndpointRules(((0, 1, 0),), (1, 2), classes=48))
    import inspect
    assert 'endpoint' not in inspect.signature(type(model).stream).parameters           # stream() keeps its parameter list
