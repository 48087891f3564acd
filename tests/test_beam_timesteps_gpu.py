"""Per-token time steps of the beam search on the device (ctc.beam_decode(return_timesteps=True), ctc.BeamSearchStream(timesteps=True),
StreamingSession decode='beam-timed'): the search itself is unchanged bit for bit, the time steps are exactly those of the plain-Python
model of the kernel's search (beam_timesteps_model.py, anchored on the oracle by test_beam_timesteps_host.py), streaming equals whole,
committed time steps are final, and the untimed stream keeps its state and its results."""
import functools
import math

import numpy as np
import pytest
import torch

import beam_timesteps_model as model
import cases
import nb_asr_amd as nb
from nb_asr_amd import ctc, frontend, hip
from nb_asr_amd.weights import keyed_fill_, keyed_input

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _rows(out, i, n_ranks=None):
    """Utterance i of a timed result as [(tokens, score, timesteps)] over its ranks; asserts the padding is 0."""
    beams, scores, steps, lens = out
    rows = []
    for r in range(beams.shape[1] if n_ranks is None else n_ranks):
        n = int(lens[i, r])
        assert torch.all(beams[i, r, n:] == 0) and torch.all(steps[i, r, n:] == 0), (i, r)
        rows.append((beams[i, r, :n].tolist(), float(scores[i, r]), steps[i, r, :n].tolist()))
    return rows


@functools.lru_cache(maxsize=None)
def _shape_results(shape):
    """{key: (log_probs, width, top_n, device rows)} of a shape's utterances, whole and ragged: one timed decode each, shared by the tests."""
    b, frames, _, width, top_n, _ = shape
    lp = model.shape_input(shape)
    dev = lp.to(DEV)
    whole = tuple(t.cpu() for t in ctc.beam_decode(dev, None, beam_width=width, cutoff_top_n=top_n, return_timesteps=True))
    lengths = model.lengths_of(b, frames)
    ragged = tuple(t.cpu() for t in ctc.beam_decode(dev, lengths, beam_width=width, cutoff_top_n=top_n, return_timesteps=True))
    out = {}
    for key, lp_i, _, _ in model.utterances(shape):
        _, kind, i = key
        out[key] = (lp_i, width, top_n, _rows(whole if kind == 'whole' else ragged, i))
    return out


@functools.lru_cache(maxsize=None)
def _narrow_results():
    out = {}
    for k, (width, _, _, lp) in enumerate(model.narrow_cases()):
        got = tuple(t.cpu() for t in ctc.beam_decode(lp.to(DEV), None, beam_width=width, return_timesteps=True))
        for i in range(2):
            out[('narrow', k, i)] = (lp[i].numpy(), width, 40, _rows(got, i))
    return out


@functools.lru_cache(maxsize=None)
def _model_beams(key):
    lp, width, top_n, _ = (_narrow_results() if key[0] == 'narrow' else _shape_results(key[0]))[key]
    return model.beam_search(lp, width, cutoff_top_n=top_n)


# ---- the search is unchanged -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('shape', model.TIMED_SHAPES)
def test_timed_search_returns_the_untimed_beams_bit_for_bit(shape):
    b, frames, _, width, top_n, _ = shape
    lp = model.shape_input(shape).to(DEV)
    for lengths in (None, model.lengths_of(b, frames)):
        beams, scores, out_len = ctc.beam_decode(lp, lengths, beam_width=width, cutoff_top_n=top_n)
        t_beams, t_scores, steps, t_len = ctc.beam_decode(lp, lengths, beam_width=width, cutoff_top_n=top_n, return_timesteps=True)
        assert torch.equal(t_beams, beams) and torch.equal(t_scores, scores) and torch.equal(t_len, out_len)
        assert steps.shape == beams.shape and steps.dtype == torch.int32 and steps.device == beams.device


# ---- the time steps are the model's ------------------------------------------------------------------------------------------------

def _compare_with_model(results):
    """Exact time steps, rank by rank.  An utterance is left out only if one of its ranks holds different tokens from the model's as a
    numerical tie (test_decode.py's _check_beams: another model beam with those tokens within 2e-4 relative score); returns how many."""
    left_out = 0
    for key, (_, width, _, rows) in results.items():
        want = _model_beams(key)
        table = {tuple(t): s for t, s, _ in want}
        tie = False
        for r, (tok, score, _) in enumerate(want):
            g_tok, g_score, _ = rows[r]
            assert abs(g_score - score) <= 2e-4 * max(1.0, abs(score)), (key, r, g_score, score)
            if g_tok != tok:
                other = table.get(tuple(g_tok))
                assert other is not None and abs(other - score) <= 2e-4 * max(1.0, abs(score)), (key, r, g_tok, tok)
                tie = True
        for r in range(len(want), width):
            assert rows[r][0] == [] and rows[r][1] > 1e38, (key, r)
        if tie:
            left_out += 1
            continue
        for r, (tok, _, steps) in enumerate(want):
            assert rows[r][2] == steps, (key, r, tok, rows[r][2], steps)
    print(f'{left_out} of {len(results)} utterances left out as numerical ties')
    assert left_out <= 0.05 * len(results)


@pytest.mark.parametrize('shape', model.TIMED_SHAPES)
def test_time_steps_equal_the_model_at_the_shapes(shape):
    """The seeds show no float32 tie in the model (test_beam_timesteps_host.py), so no utterance is expected to be left out; with at most 6
    utterances per shape the 5 % allowance admits none."""
    _compare_with_model(_shape_results(shape))


def test_time_steps_equal_the_model_on_the_narrow_beam_sweep():
    """Narrow beams over few classes: records move (rule 2) and prefixes are re-created under live extensions of their old node (rule 3) all
    the time -- test_beam_timesteps_host.py asserts both counts are positive on exactly these cases."""
    _compare_with_model(_narrow_results())


def test_time_step_properties_hold_on_the_device():
    results = dict(_narrow_results())
    for shape in model.TIMED_SHAPES:
        results.update(_shape_results(shape))
    for key, (lp, width, top_n, rows) in results.items():
        model.check_timestep_properties(key, lp, width, top_n, [row for row in rows if row[1] < 1e38])


def test_width_one_on_peaked_input_gives_the_first_frame_of_every_argmax_run():
    """A known answer, no model involved: with one beam no parent is live beside its child, every time step is the creation frame."""
    lp, path = model.peaked(3, 60)
    out = tuple(t.cpu() for t in ctc.beam_decode(lp.to(DEV), None, beam_width=1, return_timesteps=True))
    for i in range(3):
        tokens, starts = model.argmax_run_starts(path[i].tolist())
        (tok, _, steps), = _rows(out, i)
        assert tok == tokens and steps == starts and len(tokens) > 10


# ---- streaming -----------------------------------------------------------------------------------------------------------------------

def _log_probs(shape, seed, sharp=2.0):
    lp = model.log_probs(shape, seed, sharp)
    lp[:, ::3, 0] += 1.5
    return torch.log_softmax(lp, dim=2)


def _sizes(kind, t):
    if kind == 'whole':
        return [t]
    pattern = kind if isinstance(kind, tuple) else (kind,)
    sizes, i = [], 0
    while sum(sizes) < t:
        sizes.append(min(pattern[i % len(pattern)], t - sum(sizes)))
        i += 1
    return sizes


def _chunk_lengths(total, at, n):
    return None if total is None else [min(max(int(v) - at, 0), n) for v in total]


def _timed_stream(lp, sizes, width, total=None, **kw):
    """Pushes of ``sizes`` frames; returns (finish(), per utterance the concatenated committed tokens and frames, the decoder)."""
    b = lp.shape[0]
    dec = ctc.BeamSearchStream(b, beam_width=width, device=DEV, timesteps=True, **kw)
    tokens, frames, at = [[] for _ in range(b)], [[] for _ in range(b)], 0
    for n in sizes:
        committed, partial, c_frames, p_frames = dec.push(lp[:, at:at + n], _chunk_lengths(total, at, n))
        at += n
        for i in range(b):
            assert c_frames[i].dtype == torch.int32 and c_frames[i].numel() == committed[i].numel()
            assert p_frames[i].numel() == partial[i].numel()
            tokens[i] += committed[i].tolist()
            frames[i] += c_frames[i].tolist()
    assert at == lp.shape[1]
    return dec.finish(), tokens, frames, dec


def _assert_same(got, want, what):
    for g, w, name in zip(got, want, ('beams', 'scores', 'timesteps', 'out_len')):
        assert g.shape == w.shape and g.dtype == w.dtype and torch.equal(g, w), (what, name)


def _assert_committed_starts_every_finite_beam(result, tokens, frames, what):
    beams, scores, steps, _ = (t.cpu() for t in result)
    for i in range(beams.shape[0]):
        for r in range(beams.shape[1]):
            if float(scores[i, r]) < 3.0e38:
                assert beams[i, r, : len(tokens[i])].tolist() == tokens[i], (what, i, r)
                assert steps[i, r, : len(frames[i])].tolist() == frames[i], (what, i, r)


@pytest.mark.parametrize('b,frames,classes,width', [(2, 60, 49, 12), (2, 40, 4, 3)])
def test_streaming_equals_whole_bit_for_bit(b, frames, classes, width):
    lp = _log_probs((b, frames, classes), 31 * frames + width, 2.0 if classes > 5 else 1.0).to(DEV)
    saw_commit = False
    for total in (None, [frames, frames // 2]):                   # the second utterance ends early (inside a push for most chunkings)
        want = ctc.beam_decode(lp, total, beam_width=width, return_timesteps=True)
        for kind in (1, 7, (3, 0, 41, 1, 17, 5), 'whole'):
            got, tokens, c_frames, _ = _timed_stream(lp, _sizes(kind, frames), width, total)
            _assert_same(got, want, (kind, total))
            _assert_committed_starts_every_finite_beam(got, tokens, c_frames, (kind, total))
            saw_commit |= kind != 'whole' and any(len(f) for f in c_frames)
    assert saw_commit


def test_committed_time_steps_are_final_when_they_are_reported():
    """After every push, everything committed so far -- tokens and frames -- starts every finite beam of the whole search over the frames
    pushed so far: a later frame never moves a committed token's time step."""
    b, frames, classes, width = 2, 60, 49, 12
    lp = _log_probs((b, frames, classes), 31 * frames + width).to(DEV)
    dec = ctc.BeamSearchStream(b, beam_width=width, device=DEV, timesteps=True)
    tokens, c_frames, at, committed_before_the_end = [[] for _ in range(b)], [[] for _ in range(b)], 0, 0
    for n in _sizes(7, frames):
        committed, partial, new_frames, p_frames = dec.push(lp[:, at:at + n])
        at += n
        for i in range(b):
            tokens[i] += committed[i].tolist()
            c_frames[i] += new_frames[i].tolist()
        sofar = ctc.beam_decode(lp[:, :at].contiguous(), None, beam_width=width, return_timesteps=True)
        _assert_committed_starts_every_finite_beam(sofar, tokens, c_frames, at)
        beams, _, steps, lens = (t.cpu() for t in sofar)
        for i in range(b):                                         # the partial result is the best beam's rest, frames included
            n0 = int(lens[i, 0])
            assert tokens[i] + partial[i].tolist() == beams[i, 0, :n0].tolist()
            assert c_frames[i] + p_frames[i].tolist() == steps[i, 0, :n0].tolist()
        if at < frames:
            committed_before_the_end = sum(len(f) for f in c_frames)
    assert committed_before_the_end > 0


def test_pool_growth_keeps_the_records():
    b, frames, classes, width = 2, 60, 49, 12
    lp = _log_probs((b, frames, classes), 31 * frames + width).to(DEV)
    want = ctc.beam_decode(lp, None, beam_width=width, return_timesteps=True)
    got, tokens, c_frames, dec = _timed_stream(lp, _sizes(1, frames), width, pool_nodes=1 + 2 * width)
    assert dec.grown > 0 and dec.pool_nodes > 1 + 2 * width
    assert dec.state_bytes == hip.ctc_beam_stream_state_bytes(b, width, dec.pool_nodes, timesteps=True)
    _assert_same(got, want, 'grown pool')
    roomy, tokens_roomy, frames_roomy, dec_roomy = _timed_stream(lp, _sizes(1, frames), width)
    assert dec_roomy.grown == 0 and tokens == tokens_roomy and c_frames == frames_roomy
    _assert_same(got, roomy, 'grown against roomy')


def test_untimed_stream_is_untouched():
    b, frames, classes, width = 2, 60, 49, 12
    lp = _log_probs((b, frames, classes), 31 * frames + width).to(DEV)
    dec = ctc.BeamSearchStream(b, beam_width=width, device=DEV)
    assert dec.timesteps is False
    pool = 1 + width * 4 * 40
    assert dec.state_bytes == b * (64 + ((44 * width + 7) & ~7) + pool * 8) == hip.ctc_beam_stream_state_bytes(b, width, pool)
    at = 0
    for n in _sizes(7, frames):
        out = dec.push(lp[:, at:at + n])
        assert len(out) == 2
        at += n
    got, want = dec.finish(), ctc.beam_decode(lp, None, beam_width=width)
    assert len(got) == 3
    for g, w in zip(got, want):
        assert torch.equal(g, w)
    timed = ctc.BeamSearchStream(b, beam_width=width, device=DEV, timesteps=True)
    assert timed.state_bytes == b * (64 + 48 * width + pool * 16)


# ---- StreamingSession --------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _session_model():
    m = nb.get_model(cases.ARCH_M, use_rnn=True, dropout_rate=0.0)
    keyed_fill_(m, seed=1235, mode='lively')
    return m.to(DEV).eval()


def _assert_session_result(logits, result, tokens, c_frames):
    lp = ctc.log_softmax(torch.cat(logits, 1).contiguous())
    _assert_same(result, ctc.beam_decode(lp, None, return_timesteps=True), 'session')
    _assert_committed_starts_every_finite_beam(result, tokens, c_frames, 'session')
    assert result[2].shape == (lp.shape[0], 12, lp.shape[1])


def test_session_decodes_with_time_steps():
    m = _session_model()
    b, t = 2, 400
    x = keyed_input(b, t, seed=5).to(DEV)
    sess = m.stream(batch=b, max_chunk=64)
    assert sess.lookahead_frames == 178                           # tokens commit while the audio is still arriving
    logits, tokens, c_frames = [], [[] for _ in range(b)], [[] for _ in range(b)]
    with torch.no_grad():
        for at in range(0, t, 64):
            lg, committed, partial, new_frames, p_frames = sess.push(x[:, :, at:at + 64], decode='beam-timed')
            logits.append(lg)
            for i in range(b):
                assert new_frames[i].numel() == committed[i].numel() and p_frames[i].numel() == partial[i].numel()
                tokens[i] += committed[i].tolist()
                c_frames[i] += new_frames[i].tolist()
                assert all(0 <= f < sess.frames_out for f in c_frames[i] + p_frames[i].tolist())      # output-frame indices
        assert any(len(f) for f in c_frames), 'nothing committed before the flush'
        with pytest.raises(ValueError, match=r'reset\(\)'):
            sess.push(x[:, :, :4], decode='beam')                  # one utterance, one of the two searches
        with pytest.raises(ValueError, match=r'reset\(\)'):
            sess.flush(decode='beam')
        lg, result = sess.flush(decode='beam-timed')
        logits.append(lg)
        _assert_session_result(logits, result, tokens, c_frames)
        # the other way round, after reset(): the untimed search is what it was
        sess.reset()
        lg, committed, partial = sess.push(x[:, :, :300], decode='beam')
        with pytest.raises(ValueError, match=r'reset\(\)'):
            sess.push(x[:, :, 300:], decode='beam-timed')
        lg2, plain = sess.flush(decode='beam')
    want = ctc.beam_decode(ctc.log_softmax(torch.cat([lg, lg2], 1).contiguous()), None)
    for g, w in zip(plain, want):
        assert torch.equal(g, w)


def _keyed_wave(seed, samples):
    rng = np.random.default_rng(seed)
    t = np.arange(samples) / 16000.0
    tone = 0.3 * np.sin(2 * math.pi * (200.0 + 37.0 * seed) * t) + 0.2 * np.sin(2 * math.pi * 3100.0 * t)
    return torch.from_numpy((tone + 0.1 * rng.standard_normal(samples)).astype(np.float32))


def test_session_decodes_with_time_steps_from_the_waveform():
    m = _session_model()
    fe = frontend.LogMelFrontend(device=DEV)
    b = 2
    sess = m.stream(batch=b, max_chunk=64, frontend=fe)
    length = sess.lookahead_samples + 4000                        # a few thousand samples past the lookahead
    wave = torch.stack([_keyed_wave(130 + i, length) for i in range(b)]).to(DEV)
    logits, tokens, c_frames = [], [[] for _ in range(b)], [[] for _ in range(b)]
    with torch.no_grad():
        for at in range(0, length, 8000):
            lg, committed, _, new_frames, _ = sess.push_audio(wave[:, at:at + 8000], decode='beam-timed')
            logits.append(lg)
            for i in range(b):
                tokens[i] += committed[i].tolist()
                c_frames[i] += new_frames[i].tolist()
        assert sum(lg.shape[1] for lg in logits) > 0              # frames became final before the flush
        lg, result = sess.flush(decode='beam-timed')
    logits.append(lg)
    _assert_session_result(logits, result, tokens, c_frames)
