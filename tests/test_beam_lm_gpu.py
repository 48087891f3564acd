"""Bigram LM fusion of the beam search on the device (ctc.beam_decode(lm=...), ctc.BeamSearchStream(lm=...), StreamingSession(lm=...),
ctc.decode_per(lm=...)): the fused search returns the beams, lengths and time steps of the plain-Python model (beam_timesteps_model.py, anchored
on exhaustive enumeration by test_beam_lm_host.py, which also asserts that the seeds used here hold no float32 tie), an all-zero table is
the unfused search bit for bit, and streaming, peek and the session equal the whole fused search bit for bit.  Last, the binding: each
(timed, fused) combination calls exactly its plain, ``_timed`` or ``_lm`` entry points (that their arguments go by the header's names, in
its order, is test_abi.py's host check)."""
import functools

import numpy as np
import pytest
import torch

import beam_timesteps_model as model
import cases
import nb_asr_amd as nb
from nb_asr_amd import ctc, hip, streaming
from nb_asr_amd.weights import keyed_fill_, keyed_input

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _rows(out, i):
    """Utterance i of a timed result as [(tokens, score, timesteps)] over its ranks; asserts the padding is 0."""
    beams, scores, steps, lens = out
    rows = []
    for r in range(beams.shape[1]):
        n = int(lens[i, r])
        assert torch.all(beams[i, r, n:] == 0) and torch.all(steps[i, r, n:] == 0), (i, r)
        rows.append((beams[i, r, :n].tolist(), float(scores[i, r]), steps[i, r, :n].tolist()))
    return rows


def _assert_is_model(shape, W, blank=0, **lm):
    """The timed fused decode of a shape, whole and ragged, against the model with table W, rank by rank: tokens, lengths and time steps
    equal; scores within the tolerance test_beam_timesteps_gpu.py / test_decode.py use for device-against-model scores."""
    b, frames, _, width, top_n, _ = shape
    dev = model.shape_input(shape).to(DEV)
    whole = tuple(t.cpu() for t in ctc.beam_decode(dev, None, beam_width=width, blank=blank, cutoff_top_n=top_n, return_timesteps=True, **lm))
    ragged = tuple(t.cpu() for t in ctc.beam_decode(dev, model.lengths_of(b, frames), beam_width=width, blank=blank, cutoff_top_n=top_n,
                                                    return_timesteps=True, **lm))
    worst = 0.0
    for key, lp, _, _ in model.utterances(shape):
        _, kind, i = key
        rows = _rows(whole if kind == 'whole' else ragged, i)
        want = model.beam_search(lp, width, blank=blank, cutoff_top_n=top_n, fusion=W)
        for r, (tok, score, steps) in enumerate(want):
            g_tok, g_score, g_steps = rows[r]
            assert g_tok == tok, (key, r, g_tok, tok)
            assert g_steps == steps, (key, r, g_steps, steps)
            worst = max(worst, abs(g_score - score) / max(1.0, abs(score)))
            assert abs(g_score - score) <= 2e-4 * max(1.0, abs(score)), (key, r, g_score, score)
        for r in range(len(want), width):
            assert rows[r][0] == [] and rows[r][1] > 1e38, (key, r)
    print(f'{shape}: worst relative score difference {worst:.2e}')


# ---- the fused search is the model's ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('shape', model.TIMED_SHAPES)
def test_fused_search_equals_the_model_at_the_shapes(shape):
    W = model.fusion_table(shape[2])
    _assert_is_model(shape, W, lm=torch.from_numpy(W))


def test_alpha_and_beta_scale_and_shift_the_table():
    shape = (3, 40, 49, 12, 40, 2.0)
    lm = np.random.default_rng(77).normal(size=(49, 49)).astype(np.float32)
    _assert_is_model(shape, lm * np.float32(0.3) + np.float32(1.7), lm=torch.from_numpy(lm), alpha=0.3, beta=1.7)


def test_the_blank_row_is_the_start_context_wherever_blank_is():
    shape = (2, 25, 5, 4, 40, 1.0)
    W = model.fusion_table(5, seed_offset=9)
    _assert_is_model(shape, W, blank=2, lm=torch.from_numpy(W))


@pytest.mark.parametrize('shape', model.TIMED_SHAPES)
def test_a_zero_table_is_the_unfused_search_and_timed_equals_untimed_bit_for_bit(shape):
    b, frames, classes, width, top_n, _ = shape
    lp = model.shape_input(shape).to(DEV)
    zero, W = torch.zeros(classes, classes), torch.from_numpy(model.fusion_table(classes))
    for lengths in (None, model.lengths_of(b, frames)):
        for timed in (False, True):
            want = ctc.beam_decode(lp, lengths, beam_width=width, cutoff_top_n=top_n, return_timesteps=timed)
            got = ctc.beam_decode(lp, lengths, beam_width=width, cutoff_top_n=top_n, return_timesteps=timed, lm=zero)
            assert len(got) == len(want) and all(torch.equal(g, w) for g, w in zip(got, want)), (lengths, timed)
        beams, scores, out_len = ctc.beam_decode(lp, lengths, beam_width=width, cutoff_top_n=top_n, lm=W)
        t_beams, t_scores, steps, t_len = ctc.beam_decode(lp, lengths, beam_width=width, cutoff_top_n=top_n, return_timesteps=True, lm=W)
        assert torch.equal(t_beams, beams) and torch.equal(t_scores, scores) and torch.equal(t_len, out_len)
        assert steps.shape == beams.shape and steps.dtype == torch.int32


# ---- streaming -----------------------------------------------------------------------------------------------------------------------

def _log_probs(shape, seed, sharp=2.0):
    lp = model.log_probs(shape, seed, sharp)
    lp[:, ::3, 0] += 1.5
    return torch.log_softmax(lp, dim=2)


def _sizes(chunk, t):
    return [t] if chunk == 'whole' else [min(chunk, t - at) for at in range(0, t, chunk)]


def _chunk_lengths(total, at, n):
    return None if total is None else [min(max(int(v) - at, 0), n) for v in total]


def _feed(dec, lp, sizes, total=None):
    """Pushes of ``sizes`` frames -> per utterance the concatenated committed tokens."""
    tokens, at = [[] for _ in range(lp.shape[0])], 0
    for n in sizes:
        committed = dec.push(lp[:, at:at + n], _chunk_lengths(total, at, n))[0]
        at += n
        for i, c in enumerate(committed):
            tokens[i] += c.tolist()
    assert at == lp.shape[1]
    return tokens


def _assert_same(got, want, what):
    assert len(got) == len(want), what
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and g.dtype == w.dtype and torch.equal(g, w), (what, k)


def _assert_committed_starts_every_finite_beam(result, tokens, what):
    beams, scores = result[0].cpu(), result[1].cpu()
    for i in range(beams.shape[0]):
        for r in range(beams.shape[1]):
            if float(scores[i, r]) < 3.0e38:
                assert beams[i, r, : len(tokens[i])].tolist() == tokens[i], (what, i, r)


@pytest.mark.parametrize('timed', [False, True], ids=['plain', 'timed'])
@pytest.mark.parametrize('b,frames,classes,width', [(2, 40, 49, 12), (2, 40, 4, 3)])
def test_fused_streaming_equals_the_whole_fused_search_bit_for_bit(b, frames, classes, width, timed):
    lp = _log_probs((b, frames, classes), 31 * frames + width, 2.0 if classes > 5 else 1.0).to(DEV)
    W = torch.from_numpy(model.fusion_table(classes))
    saw_commit = False
    for total in (None, [frames, frames // 2]):                   # the second utterance ends early
        want = ctc.beam_decode(lp, total, beam_width=width, return_timesteps=timed, lm=W)
        unfused = ctc.beam_decode(lp, total, beam_width=width, return_timesteps=timed)
        assert not torch.equal(want[0], unfused[0])               # the table changes the beams: a stream that ignored it could not pass
        for chunk in (1, 7, 'whole'):
            dec = ctc.BeamSearchStream(b, beam_width=width, device=DEV, timesteps=timed, lm=W)
            tokens = _feed(dec, lp, _sizes(chunk, frames), total)
            got = dec.finish()
            _assert_same(got, want, (chunk, total))
            _assert_committed_starts_every_finite_beam(got, tokens, (chunk, total))
            saw_commit |= chunk != 'whole' and any(len(t) for t in tokens)
    assert saw_commit


def test_fused_stream_grows_its_pool_and_reset_keeps_the_table():
    b, frames, classes, width = 2, 40, 49, 12
    lp = _log_probs((b, frames, classes), 31 * frames + width).to(DEV)
    W = torch.from_numpy(model.fusion_table(classes))
    want = ctc.beam_decode(lp, None, beam_width=width, lm=W)
    dec = ctc.BeamSearchStream(b, beam_width=width, device=DEV, pool_nodes=1 + 2 * width, lm=W)
    table = dec.fusion
    assert table.device.type == 'cuda' and table.dtype == torch.float32 and torch.equal(table.cpu(), W)
    _feed(dec, lp, _sizes(1, frames))
    assert dec.grown > 0 and dec.pool_nodes > 1 + 2 * width
    _assert_same(dec.finish(), want, 'grown pool')
    dec.reset()
    assert dec.fusion is table
    _feed(dec, lp, _sizes(7, frames))
    _assert_same(dec.finish(), want, 'after reset()')
    with pytest.raises(ValueError, match='49 classes'):
        dec.reset()
        dec.push(lp[:, :3, :40].contiguous())                      # the table fixes the stream's classes


@pytest.mark.parametrize('timed', [False, True], ids=['plain', 'timed'])
def test_fused_peek_is_push_and_finish_on_a_twin_and_leaves_the_state(timed):
    b, classes, width = 3, 49, 12
    lp = _log_probs((b, 17 + 33, classes), 19).to(DEV)
    W = torch.from_numpy(model.fusion_table(classes))
    first, nxt, lengths = lp[:, :17], lp[:, 17:], [33, 0, 20]
    dec, twin = (ctc.BeamSearchStream(b, beam_width=width, device=DEV, timesteps=timed, lm=W) for _ in range(2))
    dec.push(first, [17, 9, 17])
    twin.push(first, [17, 9, 17])
    state = dec.state.clone()
    for chunk, lens in ((nxt, lengths), (nxt[:, :1], [1, 0, 1]), (None, None)):
        clone = ctc.BeamSearchStream(b, beam_width=width, device=DEV, timesteps=timed, lm=W)
        clone.push(first, [17, 9, 17])
        if chunk is not None:
            clone.push(chunk, lens)
        _assert_same(dec.peek(chunk, lens), clone.finish(), 'peek')
        assert torch.equal(dec.state, state)
    unfused = ctc.BeamSearchStream(b, beam_width=width, device=DEV, timesteps=timed)
    unfused.push(first, [17, 9, 17])
    assert not torch.equal(unfused.peek(nxt, lengths)[0], dec.peek(nxt, lengths)[0])
    dec.push(nxt, lengths)                                          # a peeked decoder goes on like one never peeked
    twin.push(nxt, lengths)
    _assert_same(dec.finish(), twin.finish(), 'after the peeks')


# ---- the session, the error rate -------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _session_model():
    m = nb.get_model(cases.ARCH_M, use_rnn=True, dropout_rate=0.0)
    keyed_fill_(m, seed=1235, mode='lively')
    return m.to(DEV).eval()


@pytest.mark.parametrize('decode', ['beam', 'beam-timed'])
def test_session_decodes_with_the_lm(decode):
    m = _session_model()
    b, t = 2, 200
    x = keyed_input(b, t, seed=5).to(DEV)
    W = torch.from_numpy(model.fusion_table(49))
    sess = streaming.StreamingSession(m, batch=b, max_chunk=40, lm=W, alpha=0.7, beta=0.2)      # what model.stream builds, with the LM
    logits, tokens = [], [[] for _ in range(b)]
    with torch.no_grad():
        for at in range(0, t, 40):
            lg, committed, *_ = sess.push(x[:, :, at:at + 40], decode=decode)
            logits.append(lg)
            for i in range(b):
                tokens[i] += committed[i].tolist()
        lg, result = sess.flush(decode=decode)
    logits.append(lg)
    lp = ctc.log_softmax(torch.cat(logits, 1).contiguous())
    want = ctc.beam_decode(lp, None, return_timesteps=decode == 'beam-timed', lm=W, alpha=0.7, beta=0.2)
    _assert_same(result, want, decode)
    _assert_committed_starts_every_finite_beam(result, tokens, decode)
    assert not torch.equal(want[1], ctc.beam_decode(lp, None, return_timesteps=decode == 'beam-timed')[1])      # the LM was not ignored


def test_decode_per_with_the_lm_is_the_error_rate_of_the_fused_best_beam():
    b, frames = 3, 40
    lp = _log_probs((b, frames, 49), 5).to(DEV)
    gen = torch.Generator().manual_seed(3)
    targets, targets_len = torch.randint(1, 49, (b, 12), generator=gen), torch.tensor([12, 7, 9])
    lm = ctc.bigram_lm(targets, targets_len)
    output_len = torch.tensor([frames, frames - 9, frames // 2])
    beams, _, lens = ctc.beam_decode(lp, output_len, lm=lm, alpha=2.0, beta=0.5)
    table = ctc.fold_table(48, 39).to(DEV)
    want = ctc.error_rates(beams[:, 0].contiguous(), lens[:, 0].contiguous(), targets, targets_len, blank=0, table=table).mean()
    got = ctc.decode_per(lp, output_len, targets, targets_len, lm=lm, alpha=2.0, beta=0.5)
    assert torch.equal(got, want)
    plain = ctc.beam_decode(lp, output_len)
    assert not torch.equal(plain[0][:, 0], beams[:, 0])           # with this alpha the LM moves the best beam


# ---- the binding: which entry points a combination calls ---------------------------------------------------------------------------------

def _entry_points(timed, fused):
    """What a search, then a stream's init, step, peek, step and finish call: a fused search, step or peek is ``_lm`` whether timed or not;
    init and finish have no fused form and go by the state's family."""
    chunk, state = '_lm' if fused else '_timed' if timed else '', '_timed' if timed else ''
    return [f'nbasr_ctc_beam_search{chunk}', f'nbasr_ctc_beam_stream{state}_init', f'nbasr_ctc_beam_stream{chunk}_step',
            f'nbasr_ctc_beam_stream{chunk}_peek', f'nbasr_ctc_beam_stream{chunk}_step', f'nbasr_ctc_beam_stream{state}_finish']


@pytest.mark.parametrize('fused', [False, True], ids=['unfused', 'fused'])
@pytest.mark.parametrize('timed', [False, True], ids=['plain', 'timed'])
def test_each_combination_calls_its_entry_points_and_returns_the_models_beams(timed, fused):
    """Batch 2, 6 frames, 5 classes, width 3; the second utterance ends inside the last chunk.  The input holds no float32 tie."""
    lengths, first, last = [6, 5], [4, 4], [2, 1]
    lp = model.log_probs((2, 6, 5), 1, 1.0)
    W = model.fusion_table(5) if fused else None
    lm = None if W is None else torch.from_numpy(W)
    want = [model.beam_search(lp[i, :n].numpy(), 3, fusion=W) for i, n in enumerate(lengths)]
    for i, n in enumerate(lengths):
        assert model.same_beams(want[i], model.beam_search(lp[i, :n].numpy(), 3, fusion=W, dtype=np.float64)), i
    assert not fused or any(not model.same_beams(w, model.beam_search(lp[i, :n].numpy(), 3)) for i, (w, n) in enumerate(zip(want, lengths)))
    dev, entries = lp.to(DEV), []
    hip.start_tape(entries)
    try:
        whole = ctc.beam_decode(dev, lengths, beam_width=3, return_timesteps=timed, lm=lm)
        dec = ctc.BeamSearchStream(2, beam_width=3, device=DEV, timesteps=timed, lm=lm)
        dec.push(dev[:, :4], first)
        peeked = dec.peek(dev[:, 4:], last)
        dec.push(dev[:, 4:], last)
        finished = dec.finish()
    finally:
        hip.stop_tape()
    assert dec.grown == 0 and [fn.__name__ for fn, _ in entries] == _entry_points(timed, fused)
    for fn, args in entries:
        assert len(args) == len(hip.SIGNATURES[fn.__name__][1]), fn.__name__
        if '_lm' in fn.__name__:
            assert args[-2] == int(timed) and type(args[-2]) is int, (fn.__name__, args[-2])
    _assert_same(peeked, whole, 'peek')                             # streaming is the whole search, bit for bit
    _assert_same(finished, whole, 'finish')
    assert len(whole) == (4 if timed else 3)
    beams, steps, lens = whole[0].cpu(), whole[2].cpu() if timed else None, whole[-1].cpu()
    for i, rows in enumerate(want):
        for r, (tok, _, ts) in enumerate(rows):
            n = int(lens[i, r])
            assert beams[i, r, :n].tolist() == tok and torch.all(beams[i, r, n:] == 0), (i, r)
            assert not timed or (steps[i, r, :n].tolist() == ts and torch.all(steps[i, r, n:] == 0)), (i, r)
        assert torch.all(lens[i, len(rows):] == 0)
