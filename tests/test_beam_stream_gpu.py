"""Streaming prefix beam search on the device (ctc.BeamSearchStream, nbasr_ctc_beam_stream_*): chunked equals whole bit for bit, the
committed tokens are exact and final, memory stays bounded while the pool grows when it must, and StreamingSession decodes with it."""
import numpy as np
import pytest
import torch

import cases
import nb_asr_amd as nb
from nb_asr_amd import ctc, hip
from nb_asr_amd.weights import keyed_fill_, keyed_input

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _log_probs(shape, seed, sharp=2.0):
    """Seeded log-probabilities the way test_decode.py builds them, blank boosted as in a trained model."""
    gen = torch.Generator().manual_seed(seed)
    lp = torch.log_softmax(torch.randn(*shape, generator=gen) * sharp, dim=-1)
    lp[:, ::3, 0] += 1.5
    return torch.log_softmax(lp, dim=2)


def _sizes(kind, t, seed=0):
    if kind == 'whole':
        return [t]
    if kind == 'ragged':
        rng = np.random.default_rng(seed)
        sizes = []
        while sum(sizes) < t:
            sizes.append(int(min(rng.choice([0, 0, 1, 3, 9, 17, 40]), t - sum(sizes))))
        return sizes + [0]
    return [min(kind, t - i) for i in range(0, t, kind)]


def _chunk_lengths(total, at, n):
    return None if total is None else [min(max(int(v) - at, 0), n) for v in total]


def _stream(lp, sizes, width, top_n, total=None, **kw):
    dec = ctc.BeamSearchStream(lp.shape[0], beam_width=width, cutoff_top_n=top_n, device=DEV, **kw)
    at, pushes = 0, []
    for n in sizes:
        pushes.append(dec.push(lp[:, at:at + n], _chunk_lengths(total, at, n)))
        at += n
    assert at == lp.shape[1]
    return dec.finish(), pushes, dec


def _assert_equal(got, want, what):
    for g, w, name in zip(got, want, ('beams', 'scores', 'out_len')):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape)
        assert torch.equal(g, w), (what, name)


@pytest.mark.parametrize('classes,top_n', [(49, 40), (49, 49), (5, 40), (64, 10)])
@pytest.mark.parametrize('width', [1, 4, 12, 32])
@pytest.mark.parametrize('b', [1, 5, 64])
def test_chunked_equals_whole_bit_for_bit(b, width, classes, top_n):
    frames = 50
    sharp = (0.5, 1.0, 2.0, 4.0)[(b + width + classes) % 4]
    lp = _log_probs((b, frames, classes), 1000 * b + 10 * width + classes, sharp).to(DEV)
    # per-row lengths: whole, nothing, ending inside the first push, ending halfway, ...
    total = [[frames, 0, 2, frames // 2, frames - 1, 31][i % 6] for i in range(b)]
    want_all = ctc.beam_decode(lp, None, beam_width=width, cutoff_top_n=top_n)
    want_len = ctc.beam_decode(lp, total, beam_width=width, cutoff_top_n=top_n)
    for kind in (1, 7, 64, 'whole', 'ragged'):
        sizes = _sizes(kind, frames, seed=b + width)
        got, _, _ = _stream(lp, sizes, width, top_n)
        _assert_equal(got, want_all, (kind, 'all frames'))
        got, _, _ = _stream(lp, sizes, width, top_n, total)
        _assert_equal(got, want_len, (kind, 'lengths'))


def test_narrow_beams_few_classes_sweep():
    """Prefixes drop out of narrow beams and come back (test_decode.py's narrow-beam sweep), now across chunk boundaries."""
    rng = np.random.default_rng(7)
    for case in range(30):
        width, classes, frames = int(rng.integers(2, 5)), int(rng.integers(3, 6)), int(rng.integers(20, 61))
        gen = torch.Generator().manual_seed(1000 + case)
        lp = torch.log_softmax(torch.randn(2, frames, classes, generator=gen) * float(rng.choice([0.3, 1.0, 2.0])), dim=-1).to(DEV)
        want = ctc.beam_decode(lp, None, beam_width=width)
        for kind in (1, 5, 'ragged'):
            got, _, _ = _stream(lp, _sizes(kind, frames, seed=case), width, 40)
            _assert_equal(got, want, (case, kind))


def _live_lcp(beams, scores, lens):
    seqs = [beams[r, : int(lens[r])].tolist() for r in range(beams.shape[0])
            if float(scores[r]) < 3.0e38 or int(lens[r]) > 0]
    out = []
    for toks in zip(*seqs):
        if any(t != toks[0] for t in toks):
            break
        out.append(toks[0])
    return out


@pytest.mark.parametrize('b,frames,classes,width,top_n,sharp,kind', [
    (3, 60, 49, 12, 40, 2.0, 7), (2, 80, 49, 12, 49, 4.0, 'ragged'), (2, 50, 49, 4, 40, 1.0, 1), (4, 60, 49, 32, 40, 3.0, 13)])
def test_committed_tokens_are_exact_and_final(b, frames, classes, width, top_n, sharp, kind):
    lp = _log_probs((b, frames, classes), 77 + frames, sharp).to(DEV)
    dec = ctc.BeamSearchStream(b, beam_width=width, cutoff_top_n=top_n, device=DEV)
    committed = [[] for _ in range(b)]
    at, saw_commit = 0, False
    for n in _sizes(kind, frames, seed=3):
        new, partial = dec.push(lp[:, at:at + n])
        at += n
        beams, scores, lens = (t.cpu() for t in ctc.beam_decode(lp[:, :at].contiguous(), None, beam_width=width, cutoff_top_n=top_n))
        for i in range(b):
            live = (scores[i] < 3.0e38) | (lens[i] > 0)
            assert bool(live[: int(live.sum())].all())
            assert bool((scores[i][live] < 3.0e38).all()), 'pick inputs whose survivors all have finite scores'
            committed[i] += new[i].tolist()
            saw_commit |= bool(new[i].numel())
            assert committed[i] == _live_lcp(beams[i], scores[i], lens[i]), (i, at)
            assert committed[i] + partial[i].tolist() == beams[i, 0, : int(lens[i, 0])].tolist(), (i, at)
    assert saw_commit
    beams, scores, lens = (t.cpu() for t in dec.finish())
    for i in range(b):
        for r in range(width):
            if float(scores[i, r]) < 3.0e38:
                assert beams[i, r, : len(committed[i])].tolist() == committed[i]


def _peaked(b, frames, classes=49, seed=11):
    gen = torch.Generator().manual_seed(seed)
    path = torch.randint(1, classes, (b, frames), generator=gen)
    path[:, ::2] = 0
    logits = torch.randn(b, frames, classes, generator=gen)
    logits.scatter_(2, path.unsqueeze(2), 9.0)
    return torch.log_softmax(logits, dim=2).to(DEV)


def test_memory_is_bounded_on_a_long_peaked_stream():
    """Width 1: the live beam is the committed prefix after every push, so 20 000 frames run in the initial pool.  Width 12: the pool
    holds what the live beams have not committed -- usage <= 1 + sum over the live beams of (length - committed), checked against
    beam_decode of the same prefix -- and nothing else; how far the beams diverge is the input's business ("Beam decode")."""
    b, frames, n = 4, 20000, 40
    lp = _peaked(b, frames)
    dec = ctc.BeamSearchStream(b, beam_width=1, device=DEV)
    for push, at in enumerate(range(0, frames, n)):
        committed, partial = dec.push(lp[:, at:at + n])
        assert all(p.numel() == 0 for p in partial)
        if push == 49:
            at50 = dec.state_bytes
    assert dec.state_bytes == at50 == hip.ctc_beam_stream_state_bytes(b, 1, 1 + 1 * 4 * 40) and int(dec.usage.max()) == 1
    _assert_equal(dec.finish(), ctc.beam_decode(lp, None, beam_width=1), 'width 1, 20000 frames')

    dec = ctc.BeamSearchStream(b, beam_width=12, device=DEV)
    committed = torch.zeros(b, dtype=torch.int64)
    for push, at in enumerate(range(0, frames, n)):
        new, _ = dec.push(lp[:, at:at + n])
        committed += torch.tensor([c.numel() for c in new])
        if push in (49, 199, frames // n - 1):
            _, scores, lens = (t.cpu() for t in ctc.beam_decode(lp[:, :at + n].contiguous(), None))
            pending = ((lens.long() - committed[:, None]).clamp(min=0) * ((scores < 3.0e38) | (lens > 0))).sum(1)
            assert bool((dec.usage <= 1 + pending).all()), (push, dec.usage.tolist(), pending.tolist())
    _assert_equal(dec.finish(), ctc.beam_decode(lp, None), 'width 12, 20000 frames')


def test_pool_grows_and_keeps_its_contents():
    b, frames, classes, width = 3, 300, 49, 12
    lp = _log_probs((b, frames, classes), 5, 0.3).to(DEV)              # flat: the beams diverge, pending suffixes get long
    n = 20
    got, _, dec = _stream(lp, [n] * (frames // n), width, 40, pool_nodes=1 + width * n + 1)
    assert dec.grown >= 1 and dec.pool_nodes > 1 + width * n + 1
    _assert_equal(got, ctc.beam_decode(lp, None, beam_width=width), 'grown pool')


def test_refusals():
    lp = _log_probs((2, 10, 49), 1).to(DEV)
    dec = ctc.BeamSearchStream(2, device=DEV)
    with pytest.raises(ValueError, match='expected'):
        dec.push(lp[:1])
    with pytest.raises(ValueError, match='float32'):
        dec.push(lp.double())
    with pytest.raises(ValueError, match='float32'):
        dec.push(lp.cpu())
    dec.push(lp[:, :4], [4, 2])                                    # row 1 ends inside this chunk
    with pytest.raises(ValueError, match='ended'):
        dec.push(lp[:, 4:8], [4, 1])
    with pytest.raises(ValueError, match='ended'):
        dec.push(lp[:, 4:8])
    with pytest.raises(ValueError, match='lengths'):
        dec.push(lp[:, 4:8], [5, 0])
    dec.push(lp[:, 4:8], [4, 0])
    dec.finish()
    with pytest.raises(ValueError, match='finish'):
        dec.push(lp[:, 8:])
    dec.reset()
    dec.push(lp)
    _assert_equal(dec.finish(), ctc.beam_decode(lp, None), 'after reset')
    with pytest.raises(ValueError, match='beam_width'):
        ctc.BeamSearchStream(2, beam_width=33, device=DEV)


# ---- StreamingSession --------------------------------------------------------------------------------------------------------

def _model(arch):
    m = nb.get_model(arch, use_rnn=True, dropout_rate=0.0)
    keyed_fill_(m, seed=1235, mode='lively')
    return m.to(DEV).eval()


def _session_sizes(kind, t):
    if kind == 'ragged':
        sizes, i, pattern = [], 0, (3, 0, 41, 200, 1, 17, 96, 5)
        while sum(sizes) < t:
            sizes.append(min(pattern[i % len(pattern)], t - sum(sizes)))
            i += 1
        return sizes
    return [min(kind, t - i) for i in range(0, t, kind)]


def _session_decode(sess, x, sizes):
    logits, committed, at = [], [[] for _ in range(x.shape[0])], 0
    with torch.no_grad():
        for n in sizes:
            lg, new, partial = sess.push(x[:, :, at:at + n], decode='beam')
            at += n
            logits.append(lg)
            for i, c in enumerate(new):
                committed[i] += c.tolist()
        lg, result = sess.flush(decode='beam')
    logits.append(lg)
    return torch.cat(logits, 1), committed, result


def _check_ties(got, want):
    """test_decode.py's rule: the logits of the stream and of model(x) differ by fp32 round-off, so a different beam in a rank is
    acceptable only as a numerical tie within 2e-4."""
    gb, gs, gl = (t.cpu() for t in got)
    wb, ws, wl = (t.cpu() for t in want)
    for i in range(gb.shape[0]):
        table = {tuple(wb[i, r, : int(wl[i, r])].tolist()): float(ws[i, r]) for r in range(wb.shape[1])}
        for r in range(gb.shape[1]):
            want_s = float(ws[i, r])
            assert abs(float(gs[i, r]) - want_s) <= 2e-4 * max(1.0, abs(want_s)), (i, r)
            tok = tuple(gb[i, r, : int(gl[i, r])].tolist())
            if tok != tuple(wb[i, r, : int(wl[i, r])].tolist()):
                assert tok in table and abs(table[tok] - want_s) <= 2e-4 * max(1.0, abs(want_s)), (i, r)


@pytest.mark.parametrize('kind', [1, 64, 160, 'ragged'])
@pytest.mark.parametrize('arch', ['A', 'M'])
def test_session_beam_decode(arch, kind):
    m = _model(cases.ARCHS[arch])
    b, t = 2, 300 if kind != 1 else 120
    x = keyed_input(b, t, seed=5).to(DEV)
    sess = m.stream(batch=b, max_chunk=160)
    logits, committed, result = _session_decode(sess, x, _session_sizes(kind, t))
    lp = ctc.log_softmax(logits.contiguous())
    want = ctc.beam_decode(lp, None)
    _assert_equal(result, want, (arch, kind))
    for i in range(b):
        assert result[0][i, 0, : len(committed[i])].cpu().tolist() == committed[i]
    with torch.no_grad():
        whole = ctc.beam_decode(ctc.log_softmax(m(x)), None)
    _check_ties(result, whole)


def test_session_memory_and_reset():
    m = _model(cases.ARCH_A)
    x = keyed_input(2, 300, seed=8).to(DEV)
    y = keyed_input(2, 260, seed=9).to(DEV)
    plain = m.stream(batch=2, max_chunk=64)
    before = plain.buffer_bytes
    with torch.no_grad():
        for i in range(0, 300, 64):
            plain.push(x[:, :, i:i + 64])
        plain.flush()
    assert plain.buffer_bytes == before and not plain._beams            # no beam pushes: no beam state
    sess = m.stream(batch=2, max_chunk=64)
    _, _, first = _session_decode(sess, x, [64] * 5)
    assert sess.buffer_bytes == before + sess._beams['beam'].state_bytes > before
    sess.reset()
    _, _, again = _session_decode(sess, y, [50] * 6)
    _, _, fresh = _session_decode(m.stream(batch=2, max_chunk=64), y, [50] * 6)
    _assert_equal(again, fresh, 'reset')
    # a beam decode that has missed frames is refused; so is pushing on after the flush
    sess = m.stream(batch=2, max_chunk=64)
    with torch.no_grad():
        assert sess.push(torch.cat([x, x, x], 2)).shape[1] > 0           # beyond the lookahead: logits the beam search did not see
        with pytest.raises(ValueError, match="decode='beam'"):
            sess.push(x[:, :, :10], decode='beam')
        sess.reset()
        sess.push(x[:, :, :10], decode='beam')
        sess.flush(decode='beam')
        with pytest.raises(ValueError, match='reset'):
            sess.push(x[:, :, :10], decode='beam')
