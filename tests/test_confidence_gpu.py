"""The confidence estimator on the device: the kernel against the definition (confidence_model.py) -- labels, spans, counts and every
other integer exactly, every frame's q within the derived bound of the float64 model, and the aggregation of the device's own q bit for
bit -- at the pass edges and class counts where the kernel changes path; results that do not depend on the chunking or the batch; a
peek that changes nothing; ``path_confidence`` against ``forced_align``; and streaming sessions made with ``confidence=``."""
import functools
import itertools
import json

import numpy as np
import pytest
import torch

import cases
import confidence_model as cm
import test_endpoint_gpu as eg
import test_stream_launch_sequence_gpu as sl
from nb_asr_amd import ctc, frontend, hip, streaming

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
BATCH = 5
FRAMES = (0, 1, 63, 64, 65, 128, 129, 200)
CLASSES = (2, 3, 49, 63, 64, 65, 128)
STEP = 'nbasr_ctc_confidence_step'
WORST = {}                       # measure -> the largest |q_device - q_float64| seen, in units of 2^-24 (printed; DESIGN.md 9 records it)


def rules_for(measure, classes=49, alpha=1 / 3, blank=0):
    return ctc.ConfidenceRules(measure, alpha, blank, classes, DEV)


def lengths_for(n):
    return np.array((n, 0, n // 2, max(n - 1, 0), n), dtype=np.int32)         # the full length, nothing, and in between


@functools.lru_cache(maxsize=None)
def case(n, classes):
    """(x (5, n, C) on the device with NaN beyond each row's length, the same on the host, lengths).  Values on a grid of 0.25 within
    [-2, 2], so the largest value is tied in many frames; row 0 changes label at almost every frame, row 2 has masked (-inf) classes,
    row 3's labels come in stretches of three, row 4 is all blank."""
    rng = np.random.default_rng(7000 * classes + n)
    x = (rng.integers(-8, 9, size=(BATCH, n, classes)) / 4).astype(np.float32)
    x[2][:, 1::3] = -np.inf
    stretch = np.repeat(rng.integers(0, classes, size=n // 3 + 1), 3)[:n]
    x[3][np.arange(n), stretch] = 4.0
    x[4][:, 0] = 5.0
    lengths = lengths_for(n)
    for b in range(BATCH):
        x[b, lengths[b]:] = np.nan
    x.setflags(write=False)
    return torch.from_numpy(x.copy()).to(DEV), x, lengths


def device_step(x, lengths, rules, state=None, final=True, path=None):
    """One step through the binding, trace included -> host arrays (state_out, table, counts, frame_q)."""
    b, n, _ = x.shape
    as_dev = lambda a: None if a is None else torch.as_tensor(np.asarray(a), dtype=torch.int32).to(DEV).contiguous()
    out, table = torch.empty(b, 16, dtype=torch.int32, device=DEV), torch.empty(b, n + 1, 8, dtype=torch.int32, device=DEV)
    counts, trace = torch.empty(b, dtype=torch.int32, device=DEV), torch.empty(b, n, dtype=torch.int32, device=DEV)
    hip.ctc_confidence_step(x.contiguous(), as_dev(lengths), as_dev(path), as_dev(state), out, rules.measure_index, rules.alpha, rules.blank, final,
                            table, counts, trace)
    return out.cpu().numpy(), table.cpu().numpy(), counts.cpu().numpy(), trace.cpu().numpy()


def check(x, xh, lengths, rules, path=None, state=None, final=True):
    """The device's step against the model's: the trace within the bound of the float64 model, and everything else -- the record, the
    token table, the counts -- exactly the model's integer steps over the model's labels and the device's own q."""
    got_state, got_table, got_counts, trace = device_step(x, lengths, rules, state, final, path)
    n = xh.shape[1]
    within = np.arange(n)[None, :] < (np.full(len(xh), n) if lengths is None else np.asarray(lengths))[:, None]
    assert (trace[~within] == -1).all() and (trace[within] >= 0).all() and (trace[within] <= cm.ONE).all()
    clean = np.where(within[..., None], xh, 0.0).astype(np.float32)             # (what lies beyond a row's length is never read)
    worst = cm.assert_q_close(trace, clean, lengths, rules.measure, rules.alpha, rules.blank, path)
    WORST[rules.measure] = max(WORST.get(rules.measure, 0), worst)
    print(f'{rules.measure}: C={xh.shape[2]} n={n}: at most {worst} units of 2^-24 from float64 (so far {WORST[rules.measure]})')
    if n:
        labels, _, bad = cm.frames_q(clean, rules.measure, rules.alpha, rules.blank, path)
    else:
        labels, bad = np.zeros((len(xh), 0), dtype=np.int64), np.zeros((len(xh), 0), dtype=bool)
    want_state, want_table, want_counts = cm.scan(labels, trace, lengths, state, rules.blank, final, bad)
    assert np.array_equal(got_counts, want_counts), (got_counts, want_counts)
    assert np.array_equal(got_table, want_table), (rules.measure, n, cm.tokens_of(got_table, got_counts), cm.tokens_of(want_table, want_counts))
    assert np.array_equal(got_state, want_state), (rules.measure, n, got_state, want_state)
    return got_state, got_table, got_counts, trace


def tokens_of(result):
    """Per row the 8-word entries a result's step closed, on the host; checked against the named fields."""
    table, counts = result.table.cpu().numpy(), result.counts.cpu().numpy()
    for k, name in enumerate(('labels', 'starts', 'ends', 'min_q')):
        assert np.array_equal(getattr(result, name).cpu().numpy(), table[:, :, k]), name
    for b, c in enumerate(counts):
        assert (table[b, c:] == -1).all()
    return [[tuple(int(v) for v in table[b, k]) for k in range(int(counts[b]))] for b in range(len(counts))]


# ---- the kernel against the model -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('measure', cm.MEASURES)
@pytest.mark.parametrize('n', FRAMES)
def test_kernel_equals_model_at_every_length(n, measure):
    x, xh, lengths = case(n, 49)
    rules = rules_for(measure)
    state, table, counts, trace = check(x, xh, lengths, rules)
    assert state[:, 0].tolist() == lengths.tolist() and counts[1] == 0 and counts[4] == 0 and state[4, 10] == 0        # no frames; all blank
    # the same through ctc.confidence, floats included
    result, frames = ctc.confidence(x, lengths, rules, return_frames=True)
    assert np.array_equal(result.state.cpu().numpy(), state) and np.array_equal(result.table.cpu().numpy(), table)
    assert np.array_equal(frames.cpu().numpy().view(np.int32), np.where(trace >= 0, trace.astype(np.float32) * np.float32(2.0 ** -24),
                                                                        np.float32(np.nan)).view(np.int32))
    listed = result.tokens_list()
    for b, row in enumerate(cm.tokens_of(table, counts)):
        assert listed[b] == [(label, start, end, float(cm.mean_of(s, end - start)), float(cm.min_of(m))) for label, start, end, m, s in row]
    assert torch.equal(ctc.confidence(x, lengths, rules).table, result.table)           # (without the trace)
    assert result.frames.tolist() == lengths.tolist() and result.tokens.tolist() == counts.tolist() and result.bad.tolist() == [0] * BATCH
    assert np.array_equal(result.utterance_min.cpu().numpy(), cm.min_of(state[:, 7]))
    spoken = state[:, 10] > 0
    want_mean = np.array([cm.mean_of(cm.join(r[8], r[9]), r[10]) if r[10] else np.float32(np.nan) for r in state])
    assert np.array_equal(result.utterance_mean.cpu().numpy()[spoken], want_mean[spoken]) and torch.isnan(result.utterance_mean.cpu()[~spoken]).all()


@pytest.mark.parametrize('classes', CLASSES)
def test_kernel_equals_model_at_every_class_count(classes):
    x, xh, lengths = case(129, classes)
    for measure, alpha in (('prob', 1 / 3), ('entropy', 1 / 3), ('tsallis', 1 / 3), ('tsallis', 0.5)):
        whole = check(x, xh, lengths, rules_for(measure, classes, alpha))
        for batch in (1, 3):                                     # a workgroup partly filled, or a single row
            part = device_step(x[:batch], lengths[:batch], rules_for(measure, classes, alpha))
            assert all(np.array_equal(p, w[:batch]) for p, w in zip(part, whole)), (classes, measure, batch)
    blank_last = rules_for('prob', classes, blank=classes - 1)
    check(x, xh, lengths, blank_last)


def test_the_cases_hold_what_they_are_for():
    _, xh, lengths = case(200, 49)
    top = xh[0] == xh[0].max(-1, keepdims=True)
    assert (top.sum(-1) > 1).sum() > 50                                         # frequent exact ties of the largest value
    labels = cm.greedy_labels(np.nan_to_num(xh))
    assert (labels[0] == top.argmax(-1)).all() and (np.diff(labels[0]) != 0).mean() > 0.9
    assert np.isinf(xh[2, :100]).any() and (labels[4] == 0).all() and (np.diff(labels[3, :199]) == 0).sum() > 100
    assert np.isnan(xh[2, 100:]).all() and np.abs(np.nan_to_num(xh, posinf=0, neginf=0)).max() <= 100


def planted(labels, classes=6, seed=3):
    """Logits (1, n, C) whose greedy labels are ``labels``: grid noise in [-1, 1], the label's class at 3."""
    rng = np.random.default_rng(seed)
    x = (rng.integers(-4, 5, size=(1, len(labels), classes)) / 4).astype(np.float32)
    x[0, np.arange(len(labels)), labels] = 3.0
    return torch.from_numpy(x).to(DEV), x


def test_runs_at_the_pass_boundary():
    """A run across frames 60..69; runs of one frame at lane 63 and at lane 0 of the next pass; a, blank, a around the boundary."""
    labels = np.zeros(200, dtype=np.int64)
    labels[60:70] = 2
    labels[126], labels[127], labels[128], labels[129] = 0, 4, 5, 0              # one frame at lane 63, one at lane 0
    labels[190], labels[191], labels[192] = 3, 0, 3                              # a, blank, a: two tokens
    labels[10:13] = (1, 1, 2)
    x, xh = planted(labels)
    for measure in cm.MEASURES:
        _, table, counts, _ = check(x, xh, None, rules_for(measure, 6))
        assert [t[:3] for t in cm.tokens_of(table, counts)[0]] == [(1, 10, 12), (2, 12, 13), (2, 60, 70), (4, 127, 128), (5, 128, 129), (3, 190, 191),
                                                                   (3, 192, 193)]
    for cut in (63, 64, 65, 127, 128):                           # ... and the same runs across a chunk boundary, the open token carried
        rules = rules_for('tsallis', 6)
        first = check(x[:, :cut], xh[:, :cut], None, rules, final=False)
        second = check(x[:, cut:], xh[:, cut:], None, rules, state=first[0], final=True)
        both = cm.tokens_of(first[1], first[2])[0] + cm.tokens_of(second[1], second[2])[0]
        whole = device_step(x, None, rules)
        assert both == cm.tokens_of(whole[1], whole[2])[0] and np.array_equal(second[0], whole[0])


@pytest.mark.parametrize('n', (1, 63, 64, 65, 130))
def test_a_step_can_close_frames_plus_one_tokens(n):
    """A carried token, a new label at every frame, and final: the table's last slot is used."""
    rules = rules_for('entropy', 6)
    x0, xh0 = planted(np.array([5]))
    first = check(x0, xh0, None, rules, final=False)
    assert first[2].tolist() == [0] and first[0][0, 1:3].tolist() == [5, 0]
    labels = 1 + np.arange(n) % 4
    x, xh = planted(labels, seed=n)
    state, table, counts, _ = check(x, xh, None, rules, state=first[0], final=True)
    assert counts.tolist() == [n + 1] and table.shape[1] == n + 1 and (table[0, :, 0] >= 1).all()
    assert [t[0] for t in cm.tokens_of(table, counts)[0]] == [5] + labels.tolist() and state[0, 6] == n + 1
    not_final = check(x, xh, None, rules, state=first[0], final=False)
    assert not_final[2].tolist() == [n] and (not_final[1][0, n] == -1).all() and not_final[0][0, 2] == n


def test_a_bad_path_label_counts_as_blank_and_sets_bad():
    x, xh, lengths = case(129, 49)
    rng = np.random.default_rng(9)
    path = np.repeat(rng.integers(0, 49, size=(BATCH, 44)), 3, axis=1)[:, :129]
    path[0, 64], path[0, 70], path[2, 3], path[3, 128] = 49, -1, 1000, -7         # (3, 128) lies beyond the row's length: not a frame
    path[2, 70:] = -1                                                           # beyond row 2's 64 frames: never read
    for measure in cm.MEASURES:
        state, table, counts, _ = check(x, xh, lengths, rules_for(measure), path=path)
        assert state[:, 11].tolist() == [1, 0, 1, 0, 0]
        result = ctc.confidence(x, lengths, rules_for(measure), path=torch.from_numpy(path))
        assert np.array_equal(result.state.cpu().numpy(), state) and result.bad.tolist() == [1, 0, 1, 0, 0]
    with pytest.raises(ValueError, match='path'):
        ctc.confidence(x, lengths, rules_for('prob'), path=torch.zeros(BATCH, 128))


def test_tokens_are_greedy_decodes():
    """On NaN-free input the labels are the tokens of the existing greedy kernel."""
    for n, classes in ((200, 49), (129, 128), (65, 2)):
        x, _, _ = case(n, classes)
        clean = torch.nan_to_num(x, nan=0.25).contiguous()
        want = ctc.greedy_decode(clean)
        result = ctc.confidence(clean, None, rules_for('prob', classes))
        assert [[t[0] for t in row] for row in tokens_of(result)] == [seq.tolist() for seq in want]
        assert classes == 2 or any(len(seq) > n // 2 for seq in want)


# ---- chunking, batching, peek ------------------------------------------------------------------------------------------------------
def cut(x, lengths, size):
    return [(x[:, at:at + size], np.clip(lengths - at, 0, min(size, x.shape[1] - at))) for at in range(0, x.shape[1], size)]


@pytest.mark.parametrize('measure', cm.MEASURES)
def test_chunked_equals_whole_equals_a_row_alone(measure):
    x, _, lengths = case(200, 49)
    rules = rules_for(measure)
    whole, frames = ctc.confidence(x, lengths, rules, return_frames=True)
    want_tokens, want_state = tokens_of(whole), whole.state.cpu().numpy()
    assert max(len(row) for row in want_tokens) > 100
    stream = ctc.ConfidenceStream(BATCH, rules, DEV)
    for size, finish in itertools.product((1, 7, 64, 65, 200), (False, True)):
        assert np.array_equal(stream.result.state.cpu().numpy(), cm.fresh(BATCH)) and stream.last.counts.tolist() == [0] * BATCH
        got, pieces = [[] for _ in range(BATCH)], cut(x, lengths, size)
        for i, (chunk, rows) in enumerate(pieces):
            result = stream.push(chunk, rows, final=not finish and i == len(pieces) - 1)
            assert result is stream.last and result.table.shape == (BATCH, chunk.shape[1] + 1, 8)
            got = [a + b for a, b in zip(got, tokens_of(result))]
        if finish:                                               # a final step of no frames = final=True on the last push
            assert stream.push(x[:, :0]).counts.tolist() == [0] * BATCH        # (an empty push that is not final: no launch, nothing closed)
            result = stream.finish()
            assert result.table.shape == (BATCH, 1, 8)
            got = [a + b for a, b in zip(got, tokens_of(result))]
        assert got == want_tokens, (measure, size, finish)
        assert np.array_equal(stream.last.state.cpu().numpy(), want_state) and stream.final
        with pytest.raises(ValueError, match='ended'):
            stream.push(x[:, :1])
        with pytest.raises(ValueError, match='ended'):
            stream.finish()
        stream.reset()
    for b in range(BATCH):
        alone = ctc.confidence(x[b:b + 1].contiguous(), lengths[b:b + 1], rules, return_frames=True)
        assert tokens_of(alone[0]) == want_tokens[b:b + 1] and np.array_equal(alone[0].state.cpu().numpy(), want_state[b:b + 1])
        assert torch.equal(alone[1].view(torch.int32), frames[b:b + 1].view(torch.int32))
    clean = torch.nan_to_num(x, nan=-1.0)                         # without lengths: every row takes every frame
    full = ctc.ConfidenceStream(BATCH, rules, DEV)
    got = [[] for _ in range(BATCH)]
    for chunk, _ in cut(clean, lengths, 65):
        got = [a + b for a, b in zip(got, tokens_of(full.push(chunk)))]
    got = [a + b for a, b in zip(got, tokens_of(full.finish()))]
    assert got == tokens_of(ctc.confidence(clean, None, rules)) and full.last.frames.tolist() == [200] * BATCH


def test_peek_equals_a_twins_push_and_changes_nothing():
    x, _, lengths = case(200, 49)
    rules = rules_for('tsallis')
    stream, twin = ctc.ConfidenceStream(BATCH, rules, DEV), ctc.ConfidenceStream(BATCH, rules, DEV)
    size = stream.state_bytes
    assert size == 2 * hip.ctc_confidence_state_bytes(BATCH) + BATCH * 9 * 4    # the committed record, the constant fresh one, the empty table
    assert stream.peek().counts.tolist() == [0] * BATCH                         # before any frame: nothing to close, no launch
    for chunk, rows in cut(x, lengths, 33):
        before = stream.state.clone()
        for final in (True, False):
            peeked = stream.peek(chunk, rows, final=final)
            fork = ctc.ConfidenceStream(BATCH, rules, DEV)       # a twin in the stream's committed state, pushed the chunk
            fork.state.copy_(twin.state)
            fork._fresh = twin._fresh
            pushed = fork.push(chunk, rows, final=final)
            assert tokens_of(peeked) == tokens_of(pushed) and torch.equal(peeked.state, pushed.state)
            assert torch.equal(stream.state, before)             # the committed record is only read
        at_end = stream.peek()                                   # no frames: what finish() would close now
        assert all(len(row) <= 1 for row in tokens_of(at_end)) and torch.equal(stream.state, before)
        assert tokens_of(stream.push(chunk, rows)) == tokens_of(twin.push(chunk, rows)) and torch.equal(stream.state, twin.state)
    assert stream.state_bytes == size + hip.ctc_confidence_state_bytes(BATCH)  # the peek record, made by the first peek
    assert tokens_of(stream.peek()) == tokens_of(twin.finish())


def test_stream_refusals():
    stream = ctc.ConfidenceStream(2, rules_for('prob'), DEV)
    good = torch.zeros(2, 3, 49, device=DEV)
    for bad, match in ((good[:1], 'expected'), (good[:, :, :48], 'classes'), (good.double(), 'float32'), (good.cpu(), 'HIP device')):
        with pytest.raises(ValueError, match=match):
            stream.push(bad)
        with pytest.raises(ValueError, match=match):
            stream.peek(bad)
    stream.push(good, (3, 2))
    with pytest.raises(ValueError, match='has ended'):
        stream.push(good, (1, 1))
    assert stream.push(good, (3, 0)).frames.tolist() == [6, 2]
    state = torch.empty(2, 16, dtype=torch.int32, device=DEV)
    with pytest.raises(hip.HipError, match='state_out'):
        hip.ctc_confidence_step(good, None, None, None, state[:, :8].contiguous(), 0, 0.5, 0, 1)
    with pytest.raises(hip.HipError, match='both or neither'):
        hip.ctc_confidence_step(good, None, None, None, state, 0, 0.5, 0, 1, tokens_out=torch.empty(2, 4, 8, dtype=torch.int32, device=DEV))
    with pytest.raises(hip.HipError, match='alpha'):
        hip.ctc_confidence_step(good, None, None, None, state, 2, 1.0, 0, 1)
    assert hip.ctc_confidence_step(good, None, None, None, state, 0, 0.5, 0, 1) is state and state[:, 0].tolist() == [3, 3]    # no table: the record alone


# ---- a given transcript ---------------------------------------------------------------------------------------------------------------
def test_path_confidence_returns_the_targets_with_the_aligners_spans():
    rng = np.random.default_rng(21)
    log_probs = ctc.log_softmax(torch.from_numpy(rng.standard_normal((4, 70, 49)).astype(np.float32) * 2).to(DEV))
    targets = torch.tensor([[3, 3, 7, 12, 0, 0], [5, 9, 9, 9, 2, 48], [1, 2, 3, 4, 5, 6], [8, 8, 8, 0, 0, 0]], dtype=torch.int32)
    targets_len, output_len = (4, 6, 6, 3), (70, 66, 5, 40)                    # row 2: too short for its transcript -- no path
    found = ctc.forced_align(log_probs, output_len, targets, targets_len)
    assert torch.isinf(found.score[2]) and torch.isfinite(found.score[[0, 1, 3]]).all()
    for measure in cm.MEASURES:
        result = ctc.path_confidence(log_probs, output_len, targets, targets_len, rules_for(measure))
        assert result.counts.tolist() == [4, 6, 0, 3] and result.bad.tolist() == [0] * 4 and result.frames.tolist() == [70, 66, 0, 40]
        for b, row in enumerate(tokens_of(result)):
            k = len(row)
            assert [t[0] for t in row] == targets[b, :k].tolist()
            assert [t[1] for t in row] == found.starts[b, :k].tolist() and [t[2] for t in row] == found.ends[b, :k].tolist()
        lengths = np.array(output_len, dtype=np.int32) * np.array([1, 1, 0, 1], dtype=np.int32)
        check(log_probs, log_probs.cpu().numpy(), lengths, rules_for(measure), path=found.path.cpu().numpy())
        values = result.mean[result.labels >= 0]
        assert ((values >= 0) & (values <= 1)).all() and (result.min[result.labels >= 0] <= values).all()


# ---- sessions ----------------------------------------------------------------------------------------------------------------------
def taped(call):
    entries = []
    hip.start_tape(entries)
    try:
        out = call()
    finally:
        hip.stop_tape()
    return out, [fn.__name__ for fn, _ in entries]


@pytest.mark.parametrize('audio,decode', [(False, True), (True, False)])
def test_sessions(audio, decode):
    model = sl.model_for(cases.ARCH_M, True)
    if audio:
        x, sizes = sl.waves(2, 48000, 60), (16000, 16000, 0, 12000, 4000)
        make = lambda **kw: streaming.StreamingSession(model, 2, max_chunk=64, frontend=frontend.LogMelFrontend(device=DEV), **kw)
    else:
        x, sizes = sl.features(2, 400, 6), (100, 150, 0, 90, 60)
        make = lambda **kw: streaming.StreamingSession(model, 2, max_chunk=64, beam_width=4, **kw)
    rules = rules_for('tsallis')
    with torch.no_grad():
        plain = make()
        assert plain.confidence is None
        with pytest.raises(ValueError, match='confidence'):
            plain.peek_confidence()
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
        want = ctc.confidence(whole, None, rules)
        want_tokens = tokens_of(want)
        assert emitted[0] == 0 and min(len(row) for row in want_tokens) > 4     # a push that emits nothing; tokens to speak of
        check(whole, whole.cpu().numpy(), None, rules)                         # the model's own logits, against the definition
        middle = int(np.argmax(emitted > 0))                                    # the first push that commits frames

        sess = make(confidence=rules)
        assert isinstance(sess.confidence, ctc.ConfidenceStream)
        assert sess.buffer_bytes - make().buffer_bytes == sess.confidence.state_bytes == 2 * hip.ctc_confidence_state_bytes(2) + 2 * 9 * 4
        for repeat in range(2):                                    # the second time after reset()
            assert np.array_equal(sess.confidence.last.state.cpu().numpy(), cm.fresh(2)) and sess.confidence.last.counts.tolist() == [0, 0]
            at, got = 0, [[], []]
            for i, n in enumerate(sizes):
                piece = x[..., at:at + n]
                out, names = taped(lambda: eg.feed(sess, piece, audio, decode))
                at, done = at + n, int(emitted[i])
                assert eg.same(out, plain_outs[i])                 # exactly what a session without confidence= returns
                # one more launch when frames were emitted, the last one; otherwise launch for launch the plain session
                assert names == plain_names[i] + ([STEP] if parts[i].shape[1] else [])
                got = [a + b for a, b in zip(got, tokens_of(sess.confidence.last))]
                if done:
                    so_far = ctc.confidence(whole[:, :done].contiguous(), None, rules)
                    assert all(row == full[:len(row)] and len(full) - len(row) <= 1 for row, full in zip(got, tokens_of(so_far)))
                committed = sess.confidence.state.clone()
                peeked, ahead = sess.peek_confidence(decode)
                assert eg.same(peeked, plain_peeks[i])             # peek's own result, bit for bit
                both = torch.cat([whole[:, :done], eg.logits_of(peeked)], 1).contiguous()
                assert [a + b for a, b in zip(got, tokens_of(ahead))] == tokens_of(ctc.confidence(both, None, rules))
                assert torch.equal(sess.confidence.state, committed)                    # the peek left the committed record alone
                if i == middle and repeat == 0:                    # a twin fed the same pushes and flushed now closes what the peek showed
                    twin, t_at = make(confidence=rules), 0
                    for m in sizes[:i + 1]:
                        eg.feed(twin, x[..., t_at:t_at + m], audio, decode)
                        t_at += m
                    twin.flush(decode)
                    assert tokens_of(twin.confidence.last) == tokens_of(ahead) and torch.equal(twin.confidence.last.state, ahead.state)
                    assert sum(ahead.counts.tolist()) > 0
            out, names = taped(lambda: sess.flush(decode))
            assert eg.same(out, plain_outs[-1]) and names == plain_names[-1] + [STEP]   # the final step: one launch, with or without a frame
            got = [a + b for a, b in zip(got, tokens_of(sess.confidence.last))]
            assert got == want_tokens and torch.equal(sess.confidence.last.state, want.state)
            assert sess.confidence.final
            sess.reset()


def test_all_four_listeners_step_in_order():
    sess = streaming.StreamingSession(sl.model_for(cases.ARCH_M, True), 2, confidence=rules_for('entropy'), endpoint=ctc.EndpointRules(device=DEV),
                                      keywords=ctc.KeywordSet([(3, 4)], device=DEV), segments=ctc.SegmentRules(device=DEV))
    x = sl.features(2, 400, 3)
    with torch.no_grad():
        _, quiet = taped(lambda: sess.push(x[..., :40]))
        out, names = taped(lambda: sess.push(x[..., 40:]))
        _, last = taped(lambda: sess.flush())
    steps = [STEP, 'nbasr_ctc_endpoint_step', 'nbasr_ctc_keyword_step', 'nbasr_ctc_segment_step']
    assert not set(quiet) & set(steps) and out.shape[1] > 0
    assert names[-4:] == steps and [names.count(s) for s in steps] == [1, 1, 1, 1]
    assert last[-4:] == steps and last.count(STEP) == 1
    assert int(sess.confidence.last.frames[0]) == int(sess.segments.frames[0]) == int(sess.endpoint.frames[0])


def test_session_refusals_and_the_session_without_confidence():
    model = sl.model_for(cases.ARCH_M, True)
    with pytest.raises(ValueError, match='ConfidenceRules'):
        streaming.StreamingSession(model, 1, confidence=ctc.EndpointRules())
    with pytest.raises(ValueError, match='classes'):
        streaming.StreamingSession(model, 1, confidence=ctc.ConfidenceRules(classes=48))
    # a session without confidence= makes the recorded launch sequence
    pinned = json.loads(sl.FIXTURE.read_text())
    assert sl.summarise(sl.record('greedy')) == pinned['greedy']


def test_the_largest_deviations_seen():
    """Last in the file: what the tests above saw, for DESIGN.md 9 (run with -s)."""
    print('largest |q_device - q_float64| in units of 2^-24:', WORST)
    assert all(v <= cm.CAP for v in WORST.values())
