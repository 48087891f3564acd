"""The segmenter on the device: the kernel against the definition (segment_model.py) bit for bit on every state word, every ring entry
and the mask; results that do not depend on the chunking or the batch; a peek that changes nothing; ``decode_spans`` against
``beam_decode`` of each slice alone; and streaming sessions made with ``segments=``.  The inputs are test_endpoint_gpu.py's: the
speech decision is the endpointer's."""
import numpy as np
import pytest
import torch

import cases
import endpoint_model as em
import segment_model as sm
import test_endpoint_gpu as eg
import test_stream_launch_sequence_gpu as sl
from nb_asr_amd import ctc, frontend, hip, streaming

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
BATCH = eg.BATCH
STEP = 'nbasr_ctc_segment_step'
# (min_speech, min_silence, max_frames, capacity)
RULE_SETS = (
    (1, 1, 0, 1),                # every change of the decision opens or closes: several segments within a pass, a ring that wraps
    (1, 1, 0, 2),
    (1, 1, 0, 4),
    (3, 2, 0, 4),
    (2, 5, 7, 64),               # forced closes (the all-speech row: every 7 frames)
    (2, 2, 64, 3),               # ... one of them exactly on a pass boundary: (0, 64, 1)
)


def rules_for(counts, classes=49, margin=0.0):
    return ctc.SegmentRules(*counts, speech_classes=eg.speech_set(classes), margin=margin, classes=classes, device=DEV)


def host(result):
    """(B, 8 + 4 S) int32 on the host, checked against the named fields and the ring view."""
    state = result.state.cpu().numpy()
    for k, name in enumerate(ctc.SegmentResult.FIELDS):
        assert np.array_equal(getattr(result, name).cpu().numpy(), state[:, k]), name
        assert getattr(result, name).dtype == torch.int32 and getattr(result, name).shape == (state.shape[0],)
    assert state.shape[1] == sm.state_words(result.capacity) and np.array_equal(result.ring.cpu().numpy(), sm.ring(state))
    assert np.array_equal(result.dropped.cpu().numpy(), np.maximum(state[:, 4] - result.capacity, 0))
    return state


def check_whole(n, classes, margin):
    x, _, lengths = eg.case(n, classes)
    want_mask = eg.model_mask(n, classes, margin)
    for counts in RULE_SETS:
        rules = rules_for(counts, classes, margin)
        result, mask = ctc.segment(x, lengths, rules, return_mask=True)
        want = sm.scan(want_mask, lengths, None, *counts)
        assert np.array_equal(mask.cpu().numpy(), want_mask), (n, classes, margin, counts)
        got = host(result)
        assert np.array_equal(got, want), (n, classes, margin, counts, got, want)
        assert np.array_equal(host(ctc.segment(x, lengths, rules)), want)               # (without the mask)
        assert result.spans() == sm.spans(want) and result.spans(include_open=True) == sm.spans(want, include_open=True)
    return want_mask


@pytest.mark.parametrize('margin', (0.0, 0.5))
@pytest.mark.parametrize('n', eg.FRAMES)
def test_kernel_equals_model_at_every_length(n, margin):
    mask = check_whole(n, 49, margin)
    lengths = eg.lengths_for(n)
    assert mask[3].sum() == lengths[3] and mask[4].sum() == 0                          # all speech, no speech


@pytest.mark.parametrize('margin', (0.0, 0.5))
@pytest.mark.parametrize('classes', eg.CLASSES)
def test_kernel_equals_model_at_every_class_count(classes, margin):
    check_whole(129, classes, margin)


def test_the_cases_hold_what_they_are_for():
    """Several segments closing within one pass, a ring that wraps, forced closes -- one exactly on the pass boundary -- and a row that
    never speaks."""
    _, _, lengths = eg.case(200, 49)
    mask = eg.model_mask(200, 49, 0.0)
    every = sm.scan(mask, lengths, None, 1, 1, 0, 64)
    ends = np.array([end for _, end, _ in sm.spans(every)[0]])
    assert int(every[0, 4]) > 20 and np.bincount(ends // 64).max() > 4                  # row 0: many segments, several a pass
    for capacity in (1, 2, 4):
        wrapped = sm.scan(mask, lengths, None, 1, 1, 0, capacity)
        assert wrapped[0, 4] == every[0, 4] and sm.spans(wrapped)[0] == sm.spans(every)[0][-capacity:]
    forced = sm.spans(sm.scan(mask, lengths, None, 2, 2, 64, 3), include_open=True)[3]  # the all-speech row, 199 frames
    assert forced == [(0, 64, 1), (64, 128, 1), (128, 192, 1), (192, 199, -1)]
    sevens = sm.scan(mask, lengths, None, 2, 5, 7, 64)
    assert sm.spans(sevens)[3] == [(7 * k, 7 * k + 7, 1) for k in range(28)]
    for counts in RULE_SETS:
        never = sm.scan(mask, lengths, None, *counts)[4]
        assert never[:5].tolist() == [200, 0, 200, -1, 0] and (sm.ring(never[None])[0] == sm.FRESH_ENTRY).all()


def test_rows_beyond_their_length_are_not_read_and_lengths_are_optional():
    x, _, lengths = eg.case(129, 49)
    rules = rules_for((3, 2, 0, 4))
    clean = torch.nan_to_num(x, nan=3.0)
    a, b = ctc.segment(x, lengths, rules, return_mask=True), ctc.segment(clean, lengths, rules, return_mask=True)
    assert torch.equal(a[0].state, b[0].state) and torch.equal(a[1], b[1])
    whole, mask = ctc.segment(clean, None, rules, return_mask=True)
    want, want_mask = sm.step(clean.cpu().numpy(), None, None, rules.counts, eg.speech_set(49), 0.0)
    assert np.array_equal(host(whole), want) and np.array_equal(mask.cpu().numpy(), want_mask)
    assert np.array_equal(want[:, 0], [129] * BATCH)


# ---- planted runs ------------------------------------------------------------------------------------------------------------------
def planted():
    """Two rows of 130 two-class frames.  Row 0: speech over 62..66 -- with min_speech 4 the segment starts at 62 and is decided at 65,
    in the next pass -- then silence.  Row 1: speech over 50..61, then silence across frame 64, so the close is decided in the next
    pass and lands before the boundary."""
    mask = np.zeros((2, 130), dtype=np.uint8)
    mask[0, 62:67] = 1
    mask[1, 50:62] = 1
    x = np.where(mask[..., None] == 1, np.float32([0.0, 1.0]), np.float32([1.0, 0.0])).astype(np.float32)
    return torch.from_numpy(x).to(DEV), mask


PLANTED_RULES = (4, 5, 0, 4)
PLANTED_SPANS = [[(62, 67, 0)], [(50, 62, 0)]]


def test_runs_across_the_pass_boundary():
    x, mask = planted()
    rules = ctc.SegmentRules(*PLANTED_RULES, speech_classes=(1,), classes=2, device=DEV)
    result, got_mask = ctc.segment(x, None, rules, return_mask=True)
    assert np.array_equal(got_mask.cpu().numpy(), mask)
    assert np.array_equal(host(result), sm.scan(mask, None, None, *PLANTED_RULES)) and result.spans() == PLANTED_SPANS
    upto = lambda n: ctc.segment(x[:, :n].contiguous(), None, rules)
    assert upto(65).open_start.tolist() == [-1, 50] and upto(66).open_start.tolist() == [62, 50]      # decided at 65, started at 62
    assert upto(66).count.tolist() == [0, 0] and upto(67).spans() == [[], [(50, 62, 0)]]              # the close decided at 66, ended at 62


@pytest.mark.parametrize('sizes', [(63, 2, 65), (64, 66), (65, 1, 64), (62, 4, 1, 63)])
def test_runs_across_a_chunk_boundary(sizes):
    x, mask = planted()
    rules = ctc.SegmentRules(*PLANTED_RULES, speech_classes=(1,), classes=2, device=DEV)
    stream, at, state = ctc.SegmentStream(2, rules, DEV), 0, None
    for k in sizes:
        got = host(stream.push(x[:, at:at + k]))
        state = sm.scan(mask[:, at:at + k], None, state, *PLANTED_RULES)
        assert np.array_equal(got, state), (sizes, at)
        at += k
    assert at == 130 and stream.result.spans() == PLANTED_SPANS


# ---- chunking, batching, peek ------------------------------------------------------------------------------------------------------
def cut(x, lengths, sizes):
    """[(chunk, its lengths)] of x cut into ``sizes``, the last of them repeated to the end."""
    at, out, sizes = 0, [], list(sizes)
    while at < x.shape[1]:
        k = min(sizes.pop(0) if len(sizes) > 1 else sizes[0], x.shape[1] - at)
        out.append((x[:, at:at + k], np.clip(lengths - at, 0, k)))
        at += k
    return out


@pytest.mark.parametrize('counts', [RULE_SETS[i] for i in (1, 3, 4, 5)])
def test_chunked_equals_whole_equals_a_row_alone(counts):
    x, _, lengths = eg.case(200, 49)
    mask = eg.model_mask(200, 49, 0.0)
    rules = rules_for(counts)
    whole = host(ctc.segment(x, lengths, rules))
    assert np.array_equal(whole, sm.scan(mask, lengths, None, *counts))
    stream = ctc.SegmentStream(BATCH, rules, DEV)
    for sizes in ((1,), (7,), (64,), (63, 2, 64), eg.SIZES):                # the last: empty pushes in between; after reset(), over a used state
        assert np.array_equal(host(stream.result), sm.fresh(BATCH, counts[3]))
        at, state = 0, None
        for chunk, rows in cut(x, lengths, sizes):
            got = host(stream.push(chunk, rows))
            state = sm.scan(mask[:, at:at + chunk.shape[1]], rows, state, *counts)
            at += chunk.shape[1]
            assert np.array_equal(got, state), (counts, sizes, at)
            assert got is not None and np.array_equal(got, host(stream.result))
        assert np.array_equal(got, whole), (counts, sizes)
        stream.reset()
    for b in range(BATCH):
        alone = ctc.SegmentStream(1, rules, DEV)
        for chunk, rows in cut(x, lengths, (63, 2, 64)):
            got = host(alone.push(chunk[b:b + 1].contiguous(), rows[b:b + 1]))
        assert np.array_equal(got, whole[b:b + 1]) and np.array_equal(host(ctc.segment(x[b:b + 1], lengths[b:b + 1], rules)), whole[b:b + 1])
    full = ctc.SegmentStream(BATCH, rules, DEV)                   # without lengths: every row takes every frame
    clean = torch.nan_to_num(x, nan=-1.0)
    for chunk, _ in cut(clean, lengths, (63, 2, 64)):
        got = host(full.push(chunk))
    assert np.array_equal(got, host(ctc.segment(clean, None, rules)))


@pytest.mark.parametrize('counts', [RULE_SETS[1], RULE_SETS[4]])
def test_peek_equals_a_twins_push_and_changes_nothing(counts):
    x, _, lengths = eg.case(200, 49)
    rules = rules_for(counts)
    stream, twin = ctc.SegmentStream(BATCH, rules, DEV), ctc.SegmentStream(BATCH, rules, DEV)
    size = stream.state_bytes
    assert size == 2 * hip.ctc_segment_state_bytes(BATCH, counts[3])          # the committed record and the constant fresh one
    assert np.array_equal(host(stream.peek()), sm.fresh(BATCH, counts[3]))     # before any frame
    closed_in_a_peek = 0
    for chunk, rows in cut(x, lengths, eg.SIZES):
        before = stream.state.clone()
        count = host(stream.result)[:, 4]
        peeked = host(stream.peek(chunk, rows))
        closed_in_a_peek += int((peeked[:, 4] > count).any())
        assert torch.equal(stream.state, before)                                # the committed record, ring included, is only read
        assert np.array_equal(host(stream.peek()), host(stream.result))
        pushed = host(twin.push(chunk, rows))
        assert np.array_equal(peeked, pushed)
        assert np.array_equal(host(stream.peek(chunk, rows)), pushed)           # a second peek: the same
        assert np.array_equal(host(stream.push(chunk, rows)), pushed)           # every later result: a stream that never peeked
    assert closed_in_a_peek >= 3                                                # peeks whose chunk closed segments were among them
    assert stream.state_bytes == size + hip.ctc_segment_state_bytes(BATCH, counts[3])  # the peek record, made by the first peek


def test_results_clone_and_seconds():
    x, _, lengths = eg.case(129, 49)
    stream = ctc.SegmentStream(BATCH, rules_for((1, 1, 0, 4)), DEV)
    first = stream.push(x[:, :64], np.clip(lengths, 0, 64))
    kept, was = first.clone(), host(first).copy()
    later = host(stream.push(x[:, 64:], np.clip(lengths - 64, 0, 65)))
    assert np.array_equal(host(kept), was) and not np.array_equal(later, was) and np.array_equal(host(first), later)   # a result moves, a clone stays
    open_s, starts, ends = stream.result.seconds()
    ring = sm.ring(later)
    for got, frames in ((open_s, later[:, 3]), (starts, ring[:, :, 0]), (ends, ring[:, :, 1])):
        assert got.dtype == torch.float32
        assert np.array_equal(got.cpu().numpy(), np.where(frames >= 0, frames.astype(np.float32) * np.float32(ctc.FRAME_SECONDS), np.float32(-1.0)))


def test_stream_refusals():
    stream = ctc.SegmentStream(2, rules_for((1, 1, 0, 2)), DEV)
    good = torch.zeros(2, 3, 49, device=DEV)
    for bad, match in ((good[:1], 'expected'), (good[:, :, :48], 'classes'), (good.double(), 'float32'), (good.cpu(), 'HIP device')):
        with pytest.raises(ValueError, match=match):
            stream.push(bad)
        with pytest.raises(ValueError, match=match):
            stream.peek(bad)
    stream.push(good, (3, 2))
    with pytest.raises(ValueError, match='has ended'):
        stream.push(good, (1, 1))
    assert host(stream.push(good, (3, 0)))[:, 0].tolist() == [6, 2]
    with pytest.raises(hip.HipError, match='state_out'):                        # a record of another capacity
        hip.ctc_segment_step(good, None, None, stream.state, 1, 1, 0, 3, 2, 0, 0.0)
    with pytest.raises(hip.HipError, match='capacity'):
        hip.ctc_segment_step(good, None, None, stream.state, 1, 1, 0, 65, 2, 0, 0.0)
    with pytest.raises(hip.HipError, match='max_frames'):
        hip.ctc_segment_step(good, None, None, stream.state, 2, 1, 2, 2, 2, 0, 0.0)


# ---- decode_spans ------------------------------------------------------------------------------------------------------------------
def test_decode_spans_equals_beam_decode_of_each_slice_alone():
    rng = np.random.default_rng(11)
    logits = rng.standard_normal((3, 41, 49)).astype(np.float32) * 2
    logits[:, :, list(ctc.default_speech_classes())] += 8.0                             # speech, whichever phoneme wins a frame ...
    for b, quiet in enumerate(((0, 5, 14, 19, 30, 41), (8, 12, 25, 33), (0, 41))):     # ... but for [from, to) pairs of silence; row 2: nothing said
        for lo, hi in zip(quiet[::2], quiet[1::2]):
            logits[b, lo:hi, 0] += 24.0
    log_probs = ctc.log_softmax(torch.from_numpy(logits).to(DEV))
    result = ctc.segment(log_probs, (41, 41, 41), ctc.SegmentRules(1, 2, 0, 8, device=DEV))
    spans = result.spans(include_open=True)
    assert [len(row) for row in spans] == [2, 3, 0] and spans[1][-1][2] == -1 and spans[0][0] == (5, 14, 0)
    for pad, width in ((0, 12), (2, 5), (50, 12)):
        entries = []
        hip.start_tape(entries)
        try:
            got = ctc.decode_spans(log_probs, spans, pad=pad, beam_width=width)
        finally:
            hip.stop_tape()
        assert [fn.__name__ for fn, _ in entries] == ['nbasr_ctc_beam_search']          # every span of every row in ONE search
        assert [len(row) for row in got] == [2, 3, 0]
        for b, row in enumerate(got):
            for (start, end, tokens, score), span in zip(row, spans[b]):
                assert (start, end) == span[:2] and tokens.dtype == torch.int32 and not tokens.is_cuda and isinstance(score, float)
                lo, hi = max(start - pad, 0), min(end + pad, 41)
                beams, scores, out_len = ctc.beam_decode(log_probs[b:b + 1, lo:hi].contiguous(), None, width)
                assert torch.equal(tokens, beams[0, 0, :int(out_len[0, 0])].cpu()) and len(tokens) > 0
                assert score == float(scores[0, 0])                                     # to the bit: the search is one workgroup per utterance
    entries = []
    hip.start_tape(entries)
    try:
        assert ctc.decode_spans(log_probs, [[], [], []]) == [[], [], []]
    finally:
        hip.stop_tape()
    assert entries == []                                                                # no spans: no launch


# ---- sessions ----------------------------------------------------------------------------------------------------------------------
def names_of(entries):
    return [fn.__name__ for fn, _ in entries]


def taped(call):
    entries = []
    hip.start_tape(entries)
    try:
        out = call()
    finally:
        hip.stop_tape()
    return out, names_of(entries)


SESSION_COUNTS = (1, 1, 6, 4)
SESSION_SPEECH = tuple(range(1, 49, 2))                           # the odd classes: a keyed model's logits fall on either side frame by frame


@pytest.mark.parametrize('audio,decode', [(False, True), (True, False)])
def test_sessions(audio, decode):
    model = sl.model_for(cases.ARCH_M, True)
    if audio:
        x, sizes = sl.waves(2, 48000, 60), (16000, 16000, 0, 12000, 4000)
        make = lambda **kw: streaming.StreamingSession(model, 2, max_chunk=64, frontend=frontend.LogMelFrontend(device=DEV), **kw)
    else:
        x, sizes = sl.features(2, 400, 6), (100, 150, 0, 90, 60)
        make = lambda **kw: streaming.StreamingSession(model, 2, max_chunk=64, beam_width=4, **kw)
    rules = ctc.SegmentRules(*SESSION_COUNTS, speech_classes=SESSION_SPEECH, device=DEV)
    with torch.no_grad():
        plain = make()
        assert plain.segments is None
        with pytest.raises(ValueError, match='segments'):
            plain.peek_segments()
        at, plain_outs, plain_peeks, plain_names = 0, [], [], []
        for n in sizes:
            out, names = taped(lambda: eg.feed(plain, x[..., at:at + n], audio, decode))
            plain_outs.append(out)
            plain_names.append(names)
            plain_peeks.append(plain.peek(decode))
            at += n
        out, names = taped(lambda: plain.flush(decode))
        plain_outs.append(out)
        plain_names.append(names)
        parts = [eg.logits_of(o) for o in plain_outs]
        emitted = np.cumsum([p.shape[1] for p in parts])
        whole = torch.cat(parts, 1).contiguous()
        mask = em.speech_mask(whole.cpu().numpy(), None, SESSION_SPEECH, 0.0)
        want_whole = sm.scan(mask, None, None, *SESSION_COUNTS)
        assert emitted[0] == 0 and (want_whole[:, 4] > 4).all()                         # a push that emits nothing; a ring that wraps
        middle = int(np.argmax(emitted > 0))                                            # the first push that commits frames

        sess = make(segments=rules)
        assert sess.buffer_bytes - make().buffer_bytes == sess._segments.state_bytes == 2 * hip.ctc_segment_state_bytes(2, 4)
        for repeat in range(2):                                    # the second time after reset()
            assert np.array_equal(host(sess.segments), sm.fresh(2, 4))
            at = 0
            for i, n in enumerate(sizes):
                piece = x[..., at:at + n]
                out, names = taped(lambda: eg.feed(sess, piece, audio, decode))
                at, done = at + n, int(emitted[i])
                assert eg.same(out, plain_outs[i])                 # exactly what a session without segments= returns
                # one more launch when frames were emitted, the last one; otherwise launch for launch the plain session
                assert names == plain_names[i] + ([STEP] if parts[i].shape[1] else [])
                committed = host(sess.segments)
                assert np.array_equal(committed, sm.scan(mask[:, :done], None, None, *SESSION_COUNTS))
                if done:
                    assert np.array_equal(committed, host(ctc.segment(whole[:, :done].contiguous(), None, rules)))
                peeked, ahead = sess.peek_segments(decode)
                assert eg.same(peeked, plain_peeks[i])             # peek's own result, bit for bit
                both = torch.cat([whole[:, :done], eg.logits_of(peeked)], 1).contiguous()
                want = sm.step(both.cpu().numpy(), None, None, SESSION_COUNTS, SESSION_SPEECH, 0.0)[0]
                assert np.array_equal(host(ahead), want)
                assert np.array_equal(host(sess.segments), committed)                   # the peek left the committed result alone
                if i == middle and repeat == 0:                    # a twin fed the same pushes and flushed now holds what the peek showed
                    twin, t_at = make(segments=rules), 0
                    for m in sizes[:i + 1]:
                        eg.feed(twin, x[..., t_at:t_at + m], audio, decode)
                        t_at += m
                    twin.flush(decode)
                    assert np.array_equal(host(twin.segments), want)
                    assert (want[:, 0] > committed[:, 0]).all()
            out, names = taped(lambda: sess.flush(decode))
            assert eg.same(out, plain_outs[-1]) and names == plain_names[-1] + ([STEP] if parts[-1].shape[1] else [])
            assert np.array_equal(host(sess.segments), want_whole)
            assert np.array_equal(host(ctc.segment(whole, None, rules)), want_whole)
            assert sess.segments.spans(include_open=True) == sm.spans(want_whole, include_open=True)
            sess.reset()


def test_all_three_listeners_step_in_order():
    sess = streaming.StreamingSession(sl.model_for(cases.ARCH_M, True), 2, endpoint=ctc.EndpointRules(device=DEV),
                                      keywords=ctc.KeywordSet([(3, 4)], device=DEV), segments=ctc.SegmentRules(device=DEV))
    x = sl.features(2, 400, 3)
    with torch.no_grad():
        _, quiet = taped(lambda: sess.push(x[..., :40]))
        out, names = taped(lambda: sess.push(x[..., 40:]))
    steps = ['nbasr_ctc_endpoint_step', 'nbasr_ctc_keyword_step', STEP]
    assert not set(quiet) & set(steps) and out.shape[1] > 0
    assert names[-3:] == steps and [names.count(s) for s in steps] == [1, 1, 1]
    assert int(sess.segments.frames[0]) == out.shape[1] == int(sess.endpoint.frames[0])


def test_session_refusals_and_the_session_without_segments():
    model = sl.model_for(cases.ARCH_M, True)
    with pytest.raises(ValueError, match='SegmentRules'):
        streaming.StreamingSession(model, 1, segments=ctc.EndpointRules())
    with pytest.raises(ValueError, match='classes'):
        streaming.StreamingSession(model, 1, segments=ctc.SegmentRules(1, 1, speech_classes=(1, 2), classes=48))
    # a session without segments= makes the recorded launch sequence
    import json
    pinned = json.loads(sl.FIXTURE.read_text())
    assert sl.summarise(sl.record('greedy')) == pinned['greedy']
