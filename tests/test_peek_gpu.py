"""peek on the device: ``BeamSearchStream.peek``, ``FrontendStream.peek`` and ``StreamingSession.peek`` return, bit for bit, what
``finish()`` / ``flush()`` of a twin that was fed the same way returns, and leave the peeked object as it was -- its device state, its
host attributes, and every later result.  No tolerance anywhere: both sides run the same kernels on the same values."""
import copy

import pytest
import torch

import cases
import nb_asr_amd as nb
from nb_asr_amd import ctc, frontend, hip
from nb_asr_amd.weights import keyed_fill_, keyed_input
from test_frontend_stream_gpu import keyed_wave, stats

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
HOST_ATTRS = ('usage', 'ended', 'committed', 'partial', 'committed_frames', 'partial_frames', 'frames', 'classes', 'pool_nodes', 'grown',
              '_finished', 'state_bytes')


def same(a, b):
    """Nested tuples / lists of tensors and plain values, compared exactly."""
    if isinstance(a, torch.Tensor) or isinstance(b, torch.Tensor):
        return isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor) and a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)
    if isinstance(a, (tuple, list)):
        return isinstance(b, (tuple, list)) and len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    return a == b


def snapshot(dec):
    return {k: copy.deepcopy(getattr(dec, k)) for k in HOST_ATTRS}, dec.state.clone()


def unchanged(dec, snap):
    host, state = snap
    return all(same(getattr(dec, k), v) for k, v in host.items()) and torch.equal(dec.state, state)


def noise_log_probs(batch, frames, classes, seed):
    gen = torch.Generator().manual_seed(seed)
    return torch.log_softmax(2.0 * torch.randn(batch, frames, classes, generator=gen), 2).to(DEV)


def decoder(batch, width, cutoff, timed, pool_nodes=None):
    return ctc.BeamSearchStream(batch, width, 0, cutoff, DEV, pool_nodes=pool_nodes, timesteps=timed)


# ---- 1. the beam search -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('timed', [False, True], ids=['plain', 'timed'])
@pytest.mark.parametrize('cutoff', [40, 5])
@pytest.mark.parametrize('width', [1, 12, 32])
@pytest.mark.parametrize('batch,classes', [(1, 49), (3, 49), (5, 3), (2, 64)])
def test_beam_peek_is_push_and_finish_on_a_twin(batch, classes, width, cutoff, timed):
    history, nexts = (0, 1, 17, 40), (0, 1, 33)
    lp = noise_log_probs(batch, sum(history) + max(nexts), classes, 100 * batch + classes + width)
    dec, plain = decoder(batch, width, cutoff, timed), decoder(batch, width, cutoff, timed)
    at, fed = 0, []
    for n in history:
        fed.append(lp[:, at:at + n])
        assert same(dec.push(fed[-1]), plain.push(fed[-1])), n          # a peeked decoder goes on like one never peeked
        at += n
        for nxt in nexts:
            twin = decoder(batch, width, cutoff, timed)
            for chunk in fed:
                twin.push(chunk)
            twin.push(lp[:, at:at + nxt])
            want = twin.finish()
            snap = snapshot(dec)
            got = dec.peek(lp[:, at:at + nxt])
            assert same(got, want), (n, nxt)
            assert unchanged(dec, snap), (n, nxt)
            if nxt == 0:
                assert same(dec.peek(), want) and unchanged(dec, snap)
    assert same(dec.finish(), plain.finish())
    with pytest.raises(ValueError, match='push after finish'):
        dec.peek()


@pytest.mark.parametrize('timed', [False, True], ids=['plain', 'timed'])
def test_beam_peek_with_ragged_lengths(timed):
    """Utterance 1 ends in the history (9 of 17 frames) and takes nothing more; utterance 2 ends inside the peeked chunk."""
    batch, width = 3, 12
    lp = noise_log_probs(batch, 17 + 33 + 5, 49, 7)
    first, nxt, rest = lp[:, :17], lp[:, 17:50], lp[:, 50:]
    len_first, len_next, len_rest = [17, 9, 17], [33, 0, 20], [5, 0, 0]
    dec, plain, twin = (decoder(batch, width, 40, timed) for _ in range(3))
    assert same(dec.push(first, len_first), plain.push(first, len_first))
    twin.push(first, len_first)
    twin.push(nxt, len_next)
    snap = snapshot(dec)
    assert same(dec.peek(nxt, len_next), twin.finish())
    assert unchanged(dec, snap)
    with pytest.raises(ValueError, match='has ended'):
        dec.peek(nxt)                                                # utterance 1 cannot take 33 more frames: push refuses that too
    with pytest.raises(ValueError, match='has ended'):
        dec.peek(nxt, [33, 1, 20])
    assert unchanged(dec, snap)
    assert same(dec.push(nxt, len_next), plain.push(nxt, len_next))
    assert same(dec.peek(rest, len_rest), dec.peek(rest, len_rest))
    with pytest.raises(ValueError, match='has ended'):
        dec.peek(rest, [5, 0, 1])
    assert same(dec.finish(), plain.finish())


@pytest.mark.parametrize('timed', [False, True], ids=['plain', 'timed'])
def test_beam_peek_never_grows_the_pool(timed):
    """pool_nodes such that usage + width * n + 1 == pool_nodes + 1: a push of the chunk has to grow the pool, a peek of it must not."""
    batch, width, n = 2, 12, 33
    lp = noise_log_probs(batch, 20 + n, 49, 11)
    probe = decoder(batch, width, 40, timed)
    for i in range(10):
        probe.push(lp[:, 2 * i:2 * i + 2])
    pool = int(probe.usage.max()) + width * n
    dec, twin = decoder(batch, width, 40, timed, pool_nodes=pool), decoder(batch, width, 40, timed, pool_nodes=pool)
    for i in range(10):
        dec.push(lp[:, 2 * i:2 * i + 2])
        twin.push(lp[:, 2 * i:2 * i + 2])
    assert dec.grown == 0 and dec.pool_nodes == pool and int(dec.usage.max()) + width * n + 1 == pool + 1
    snap = snapshot(dec)
    got = dec.peek(lp[:, 20:])
    twin.push(lp[:, 20:])
    assert twin.grown == 1 and twin.pool_nodes > pool
    assert same(got, twin.finish())
    assert unchanged(dec, snap) and dec.grown == 0 and dec.pool_nodes == pool


# ---- 2. - 3. sessions fed features ----------------------------------------------------------------------------------------------------
def build(arch, use_rnn):
    m = nb.get_model(arch, use_rnn=use_rnn, dropout_rate=0.0)
    keyed_fill_(m, seed=1235, mode='lively')
    return m.to(DEV).eval()


def pieces_of(x, sizes):
    out, at = [], 0
    for n in sizes:
        out.append(x[:, :, at:at + n])
        at += n
    assert at == x.shape[2]
    return out


def twin_flush(twin, pieces, decode=False, audio=False):
    """flush() of a session that was fed ``pieces`` from its start (one twin per test, reset for every use)."""
    twin.reset()
    for p in pieces:
        (twin.push_audio if audio else twin.push)(p, decode=decode)
    return twin.flush(decode=decode)


@pytest.mark.parametrize('arch,use_rnn,b,t,max_chunk,sizes', [
    ('M', True, 2, 700, 64, (50, 1, 0, 130, 7, 300, 212)),
    ('D', True, 1, 600, 160, (160, 160, 160, 120)),
    ('A', False, 2, 560, 160, (40,) * 14),
])
def test_session_peek_is_flush_on_a_twin(arch, use_rnn, b, t, max_chunk, sizes):
    m = build(cases.ARCHS[arch], use_rnn)
    pieces = pieces_of(keyed_input(b, t, seed=3).to(DEV), sizes)
    sess, plain, twin = (m.stream(batch=b, max_chunk=max_chunk) for _ in range(3))
    got, want, emitted_early = [], [], False
    with torch.no_grad():
        assert sess.peek().shape == (b, 0, 49) and sess.frames_in == 0
        for i, p in enumerate(pieces):
            got.append(sess.push(p))
            want.append(plain.push(p))
            emitted_early |= sess.frames_out > 0
            provisional = sess.peek()
            assert provisional.shape == (b, hip.output_frames(sess.frames_in) - sess.frames_out, 49), i
            assert torch.equal(provisional, twin_flush(twin, pieces[:i + 1])), i
            assert torch.equal(sess.peek(), provisional), i
            assert (sess.frames_in, sess.frames_out) == (plain.frames_in, plain.frames_out)
        got.append(sess.flush())
        want.append(plain.flush())
    assert emitted_early                                                # peeks in mid-stream too, not only before the first emitted frame
    assert all(torch.equal(g, w) for g, w in zip(got, want))
    assert torch.equal(torch.cat(got, 1), torch.cat(want, 1)) and sess.frames_out == hip.output_frames(t)


@pytest.mark.parametrize('decode', [True, 'beam', 'beam-timed'])
def test_session_peek_decodes_like_flush(decode):
    b, t, sizes = 3, 700, (50, 1, 0, 130, 7, 300, 212)
    m = build(cases.ARCH_M, True)
    pieces = pieces_of(keyed_input(b, t, seed=9).to(DEV), sizes)
    sess, plain, twin = (m.stream(batch=b, max_chunk=64) for _ in range(3))
    with torch.no_grad():
        assert same(sess.peek(decode=decode), twin.flush(decode=decode))           # before any frame: the empty hypotheses
        assert not sess._beams and sess._beam_mode is None
        for i, p in enumerate(pieces):
            assert same(sess.push(p, decode=decode), plain.push(p, decode=decode)), i
            mode = sess._beam_mode
            want = twin_flush(twin, pieces[:i + 1], decode)
            assert same(sess.peek(decode=decode), want), i
            assert same(sess.peek(decode=decode), want), i
            assert sess._beam_mode == mode and torch.equal(sess.prev_token, plain.prev_token)
        assert same(sess.flush(decode=decode), plain.flush(decode=decode))


def test_session_peek_refusals():
    m = build(cases.ARCH_M, True)
    x = keyed_input(2, 400, seed=4).to(DEV)
    sess = m.stream(batch=2, max_chunk=160)
    with torch.no_grad():
        sess.push(x[:, :, :100])
        assert sess.frames_out == 0
        sess.peek(decode='beam')                                    # no frame emitted yet: the search may still start
        assert sess._beam_mode is None
        sess.push(x[:, :, 100:])
        assert sess.frames_out > 0
        with pytest.raises(ValueError, match='every logit frame'):
            sess.peek(decode='beam')                                # as push(decode='beam') is refused now
        with pytest.raises(ValueError, match='every logit frame'):
            sess.push(x[:, :, :0], decode='beam')
        sess.peek()
        sess.flush()
        with pytest.raises(ValueError, match='reset'):
            sess.peek()
        sess.reset()
        sess.push(x[:, :, :200], decode='beam-timed')
        with pytest.raises(ValueError, match="after decode='beam-timed'"):
            sess.peek(decode='beam')
        sess.peek(decode='beam-timed')
        sess.reset()
        sess.push(x[:, :, :100])
        m.model[0].conv.weight.mul_(1.0)
    with pytest.raises(ValueError, match='changed'):
        sess.peek()


# ---- 4. from the waveform -------------------------------------------------------------------------------------------------------------
AUDIO_SIZES = (1, 199, 1, 2360, 160, 8000)


def wave_pieces(b):
    wave = torch.stack([keyed_wave(90 + i, sum(AUDIO_SIZES)) for i in range(b)]).to(DEV)
    out, at = [], 0
    for n in AUDIO_SIZES:
        out.append(wave[:, at:at + n])
        at += n
    return out


def test_audio_session_peek_is_flush_on_a_twin():
    b = 2
    mean, var = stats()
    fe = frontend.LogMelFrontend(mean=mean, variance=var, device=DEV)
    m = build(cases.ARCH_M, True)
    pieces = wave_pieces(b)
    sess, plain, twin = (m.stream(batch=b, frontend=fe) for _ in range(3))
    got, want, fed = [], [], 0
    with torch.no_grad():
        assert sess.peek().shape == (b, 0, 49)
        for i, p in enumerate(pieces):
            got.append(sess.push_audio(p))
            want.append(plain.push_audio(p))
            fed += p.shape[1]
            fs = sess._frontend
            tails, counts = fs._tails.clone(), (fs.samples_in, fs.frames_out, fs._turn, fs._tail_first, fs._tail_len, sess.frames_in)
            provisional = sess.peek()
            if fed <= 200:
                assert provisional.shape == (b, 0, 49), i
            else:
                assert provisional.shape == (b, hip.output_frames(fed // 160 + 1) - sess.frames_out, 49), i
                assert torch.equal(provisional, twin_flush(twin, pieces[:i + 1], audio=True)), i
                assert torch.equal(sess.peek(), provisional), i
            assert torch.equal(fs._tails, tails) and counts == (fs.samples_in, fs.frames_out, fs._turn, fs._tail_first, fs._tail_len, sess.frames_in)
        got.append(sess.flush())
        want.append(plain.flush())
    assert all(torch.equal(g, w) for g, w in zip(got, want))


def test_audio_session_peek_with_chunks_of_one_frame():
    """max_chunk 1: the front-end's two end frames are two uncommitted pushes before the final step."""
    b = 1
    fe = frontend.LogMelFrontend(device=DEV)
    m = build(cases.ARCH_M, True)
    wave = keyed_wave(95, 1700)[None].to(DEV)
    pieces = [wave[:, :900], wave[:, 900:1440], wave[:, 1440:]]              # 1440 = 9 hops: a flush there emits 2 frames
    sess, plain, twin = (m.stream(batch=b, max_chunk=1, frontend=fe) for _ in range(3))
    with torch.no_grad():
        for i, p in enumerate(pieces):
            assert torch.equal(sess.push_audio(p), plain.push_audio(p))
            assert torch.equal(sess.peek(), twin_flush(twin, pieces[:i + 1], audio=True)), i
        assert frontend.frames_peek(1440) == 2
        assert torch.equal(sess.flush(), plain.flush())


def test_frontend_peek_is_flush_on_a_twin():
    b = 2
    mean, var = stats()
    fe = frontend.LogMelFrontend(mean=mean, variance=var, device=DEV)
    pieces = wave_pieces(b)
    fs, plain = fe.stream(b), fe.stream(b)
    fed = 0
    for i, p in enumerate(pieces):
        assert torch.equal(fs.push(p), plain.push(p)), i
        fed += p.shape[1]
        tails, counts = fs._tails.clone(), (fs.samples_in, fs.frames_out, fs._turn, fs._tail_first, fs._tail_len, fs.state_bytes)
        got = fs.peek()
        if fed <= 200:
            assert got.shape == (b, 80, 0)
        else:
            twin = fe.stream(b)
            for q in pieces[:i + 1]:
                twin.push(q)
            want = twin.flush()
            assert want.shape[2] == frontend.frames_peek(fed) and torch.equal(got, want), i
            staging = torch.zeros(b, 80, 8, device=DEV)
            assert torch.equal(fs.peek(out=(staging, 4)), want) and torch.equal(staging[:, :, 4:4 + want.shape[2]], want)
        assert torch.equal(fs._tails, tails) and counts == (fs.samples_in, fs.frames_out, fs._turn, fs._tail_first, fs._tail_len, fs.state_bytes)
        assert fs.state_bytes == 2 * 404 * 4 * b
    assert torch.equal(fs.flush(), plain.flush())
    with pytest.raises(ValueError, match='reset'):
        fs.peek()


# ---- 5. memory ----------------------------------------------------------------------------------------------------------------------
def test_peek_memory_is_allocated_once_and_only_by_a_peek():
    b, chunk = 2, 40
    m = build(cases.ARCH_M, True)
    x = keyed_input(b, chunk * 30, seed=5).to(DEV)
    sess, never = m.stream(batch=b, max_chunk=chunk), m.stream(batch=b, max_chunk=chunk)
    start = never.buffer_bytes
    assert sess.buffer_bytes == start
    marks = {}
    with torch.no_grad():
        for i in range(30):
            p = x[:, :, i * chunk:(i + 1) * chunk]
            never.push(p, decode='beam')
            sess.push(p, decode='beam')
            before = sess.buffer_bytes
            sess.peek()
            sess.peek(decode='beam')
            assert i == 0 or sess.buffer_bytes == before             # only the first peeks allocate
            if i in (2, 29):
                torch.cuda.synchronize()
                marks[i] = (sess.buffer_bytes, torch.cuda.memory_allocated(DEV))
    assert sess.frames_out > 0
    assert marks[2] == marks[29]
    assert never.buffer_bytes == start + never._beams['beam'].state_bytes and never._peek is None and never._beams['beam'].peek_bytes == 0
    assert sess.buffer_bytes > never.buffer_bytes
