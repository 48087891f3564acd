"""Incremental front-end on the device (frontend.FrontendStream, nbasr_frontend_stream_step) and the session that takes the waveform
(StreamingSession.push_audio): the streamed frames against the oracle and against the whole-utterance chain under the tolerances of
tests/test_frontend.py, bit-identical across chunkings and batches, bounded state, and exact plumbing into the model's session."""
import math
import pathlib

import numpy as np
import pytest
import torch

import cases
import nb_asr_amd as nb
from nb_asr_amd import frontend, hip
from nb_asr_amd.weights import keyed_fill_
from oracle import frontend_oracle as fo

pytestmark = pytest.mark.gpu
GOLDEN = pathlib.Path(__file__).resolve().parent / 'golden' / 'frontend_fixtures.npz'
DEV = 'cuda:0'


def keyed_wave(seed, samples):
    rng = np.random.default_rng(seed)
    t = np.arange(samples) / 16000.0
    tone = 0.3 * np.sin(2 * math.pi * (200.0 + 37.0 * seed) * t) + 0.2 * np.sin(2 * math.pi * 3100.0 * t)
    return torch.from_numpy((tone + 0.1 * rng.standard_normal(samples)).astype(np.float32))


def stats():
    z = np.load(GOLDEN)
    return z['moving_mean'], z['moving_variance']


def sizes_of(kind, length):
    if kind == 'whole':
        return [length]
    if kind == 'ragged':
        sizes, pattern, i = [], (3, 0, 411, 160, 1, 1000, 17, 0, 96), 0
        while sum(sizes) < length:
            sizes.append(min(pattern[i % len(pattern)], length - sum(sizes)))
            i += 1
        return sizes
    return [min(kind, length - i) for i in range(0, length, kind)]


def kinds_for(length):
    return ([1] if length <= 1600 else []) + [160, 400, 1000, 'ragged', 'whole']


def streamed(fs, wave, sizes):
    """Pushes of ``sizes`` samples then flush: (the list of feature chunks, each checked against the frame-count rule)."""
    outs, at = [], 0
    for n in sizes:
        before = fs.frames_out
        f = fs.push(wave[:, at:at + n])
        at += n
        assert fs.samples_in == at and f.shape[2] == frontend.frames_final(at) - before == fs.frames_out - before
        outs.append(f)
    assert at == wave.shape[1]
    last = fs.flush()
    assert last.shape[2] in (1, 2) and fs.frames_out == at // 160 + 1
    return outs + [last]


def oracle_pair(waves, mean=None, var=None):
    want, _ = fo.features(waves, mean, var)
    truth, _ = fo.features(waves, mean, var, dtype=torch.float64)
    return want, truth


def assert_frontend_tolerances(got, want, truth):
    """The rule of tests/test_frontend.py::test_frontend_matches_oracle."""
    assert tuple(got.shape) == tuple(want.shape) and torch.isfinite(got).all()
    err_hip = float((got.double() - truth).abs().max())
    err_cpu = float((want.double() - truth).abs().max())
    print(f'max error vs fp64: streamed {err_hip:.3e}, fp32 oracle {err_cpu:.3e}')
    assert err_hip <= max(3.0 * err_cpu, 2e-5), (err_hip, err_cpu)
    torch.testing.assert_close(got, want, rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize('length,b', [(16000, 2), (9999, 3), (12345, 1), (1600, 2), (401, 3)])
def test_streamed_features_match_the_oracle(length, b):
    mean, var = stats()
    waves = [keyed_wave(10 + i, length) for i in range(b)]
    want, truth = oracle_pair(waves, mean, var)
    fe = frontend.LogMelFrontend(mean=mean, variance=var, device=DEV)
    wave = torch.stack(waves).to(DEV)
    fs = fe.stream(b)
    for kind in kinds_for(length):
        fs.reset()
        got = torch.cat(streamed(fs, wave, sizes_of(kind, length)), 2).cpu()
        assert tuple(got.shape) == (b, 80, length // 160 + 1), kind
        assert_frontend_tolerances(got, want, truth)


@pytest.mark.parametrize('length', [401, 1600, 12345])
def test_every_chunking_gives_the_same_bits(length):
    mean, var = stats()
    fe = frontend.LogMelFrontend(mean=mean, variance=var, device=DEV)
    wave = torch.stack([keyed_wave(40 + i, length) for i in range(64)]).to(DEV)
    fs = fe.stream(64)
    ref = torch.cat(streamed(fs, wave, [length]), 2)
    for kind in kinds_for(length):
        if kind == 1 and length > 401:
            continue
        fs.reset()
        assert torch.equal(torch.cat(streamed(fs, wave, sizes_of(kind, length)), 2), ref), kind
    for lane in (0, 37, 63):                                        # one utterance alone = the same utterance as a lane of 64
        one = fe.stream(1)
        for kind in ('whole', 400, 'ragged'):
            one.reset()
            assert torch.equal(torch.cat(streamed(one, wave[lane:lane + 1], sizes_of(kind, length)), 2), ref[lane:lane + 1]), (lane, kind)


@pytest.mark.parametrize('length,b', [(16000, 2), (9999, 3), (401, 1)])
def test_streamed_features_match_the_whole_utterance_chain(length, b):
    mean, var = stats()
    waves = [keyed_wave(50 + i, length) for i in range(b)]
    _, truth = oracle_pair(waves, mean, var)
    fe = frontend.LogMelFrontend(mean=mean, variance=var, device=DEV)
    wave = torch.stack(waves).to(DEV)
    whole = fe(wave).cpu()
    got = torch.cat(streamed(fe.stream(b), wave, sizes_of(1000, length)), 2).cpu()
    assert_frontend_tolerances(got, whole, truth)


def test_without_normalisation_and_into_a_callers_buffer():
    length, b = 4000, 2
    waves = [keyed_wave(60 + i, length) for i in range(b)]
    want, truth = oracle_pair(waves)
    fe = frontend.LogMelFrontend(device=DEV)                        # plain log-mel
    wave = torch.stack(waves).to(DEV)
    plain = torch.cat(streamed(fe.stream(b), wave, sizes_of(400, length)), 2)
    assert_frontend_tolerances(plain.cpu(), want, truth)
    # out=: exactly the named columns are written
    fs = fe.stream(b)
    buf = torch.full((b, 80, 40), float('nan'), device=DEV)
    col, at = 5, 0
    for n in (1000, 0, 1800, 1200):
        view = fs.push(wave[:, at:at + n], out=(buf, col))
        at += n
        assert view.shape[2] == fs.frames_out - (col - 5) and view.shape[:2] == (b, 80)
        col += view.shape[2]
    col += fs.flush(out=(buf, col)).shape[2]
    assert col == 5 + length // 160 + 1 == 31
    assert torch.equal(buf[:, :, 5:31], plain)
    assert torch.isnan(buf[:, :, :5]).all() and torch.isnan(buf[:, :, 31:]).all()
    with pytest.raises(ValueError, match='do not fit'):
        fe.stream(b).push(wave, out=(buf, 20))
    with pytest.raises(ValueError, match='out must be'):
        fe.stream(b).push(wave, out=(torch.empty(b, 80, 30, device=DEV), 0))


def test_stream_state_is_fixed():
    b = 4
    fe = frontend.LogMelFrontend(device=DEV)
    wave = torch.stack([keyed_wave(70 + i, 1600 * 200) for i in range(b)]).to(DEV)
    fs = fe.stream(b)
    assert fs.state_bytes == 2 * 404 * 4 * b == hip.frontend_stream_state_bytes(b, 400)
    for i in range(200):
        fs.push(wave[:, i * 1600:(i + 1) * 1600])
        if i in (9, 199):
            torch.cuda.synchronize()
            used = torch.cuda.memory_allocated(DEV)
            if i == 9:
                at10 = used
    assert used == at10
    assert fs.frames_out == frontend.frames_final(1600 * 200) and fs._tail_len <= 400


def build(arch, mode='xavier'):
    m = nb.get_model(arch, use_rnn=True, dropout_rate=0.0)
    keyed_fill_(m, seed=1235, mode=mode)
    return m.to(DEV).eval()


def test_push_audio_is_push_of_the_streamed_features():
    mean, var = stats()
    fe = frontend.LogMelFrontend(mean=mean, variance=var, device=DEV)
    m = build(cases.ARCH_A, 'lively')
    b, length = 3, 24000
    wave = torch.stack([keyed_wave(80 + i, length) for i in range(b)]).to(DEV)
    sizes = [1600, 0, 150, 8000, 37, 4000, 213, 10000]
    assert sum(sizes) == length
    for decode in (False, True, 'beam'):
        audio = m.stream(batch=b, max_chunk=32, frontend=fe)
        plain = m.stream(batch=b, max_chunk=32)
        assert audio.lookahead_samples == 200 + 160 * audio.lookahead_frames and plain.lookahead_samples is None
        assert audio.buffer_bytes == plain.buffer_bytes + 2 * 404 * 4 * b + b * 80 * 32 * 4
        fs = fe.stream(b)
        got, want, at = [], [], 0
        with torch.no_grad():
            for n in sizes:
                got.append(audio.push_audio(wave[:, at:at + n], decode=decode))
                want.append(plain.push(fs.push(wave[:, at:at + n]), decode=decode))
                at += n
            tail = plain.push(fs.flush(), decode=decode)
            got.append(audio.flush(decode=decode))
            want_flush = plain.flush(decode=decode)
        first = lambda r: r if isinstance(r, torch.Tensor) else r[0]
        g = torch.cat([first(r) for r in got], 1)
        w = torch.cat([first(r) for r in want] + [first(tail), first(want_flush)], 1)
        assert g.shape[1] == hip.output_frames(length // 160 + 1) == audio.frames_out and torch.equal(g, w), decode
        for gp, wp in zip(got[:-1], want):                          # push by push, not only in total
            assert torch.equal(first(gp), first(wp))
        if decode is True:
            for i in range(b):
                tokens = lambda rs: [t for r in rs for t in r[1][i].tolist()]
                assert tokens(got) == tokens(want + [tail, want_flush])
        if decode == 'beam':
            for i in range(b):
                committed = lambda rs: [t for r in rs for t in r[1][i].tolist()]
                assert committed(got[:-1]) == committed(want + [tail])
            for x, y in zip(got[-1][1], want_flush[1]):
                assert torch.equal(x, y)


@pytest.mark.parametrize('kind', [1600, 4000, 'ragged'])
def test_streamed_audio_matches_the_whole_forward(kind):
    from oracle import asr_oracle as oracle
    mean, var = stats()
    fe = frontend.LogMelFrontend(mean=mean, variance=var, device=DEV)
    m = build(cases.ARCH_D)
    b, length = 2, 64000
    wave = torch.stack([keyed_wave(90 + i, length) for i in range(b)]).to(DEV)
    sess = m.stream(batch=b, frontend=fe)
    outs, at = [], 0
    with torch.no_grad():
        for n in sizes_of(kind, length):
            outs.append(sess.push_audio(wave[:, at:at + n]))
            at += n
        outs.append(sess.flush())
        x = torch.cat(streamed(fe.stream(b), wave, [length]), 2).contiguous()
        whole = m(x).cpu()
    got = torch.cat(outs, 1)
    assert sess.frames_out == hip.output_frames(length // 160 + 1) == got.shape[1] and sess.frames_in == length // 160 + 1
    truth = oracle.asr_forward(dict(m.state_dict()), cases.ARCH_D, x.cpu(), use_rnn=True, dtype=torch.float64)
    cases.assert_parity(got, whole, truth, f'audio pushes {kind}')


def test_refusals_on_the_device():
    fe = frontend.LogMelFrontend(device=DEV)
    w = torch.stack([keyed_wave(120, 1000), keyed_wave(121, 1000)]).to(DEV)
    fs = fe.stream(2)
    assert fs.push(w[:, :200]).shape == (2, 80, 0)
    with pytest.raises(ValueError, match='more than 200 samples'):
        fs.flush()
    assert fs.push(w[:, 200:201]).shape == (2, 80, 1)                # frame 0 is final at 201 samples
    assert fs.flush().shape == (2, 80, 1)
    with pytest.raises(ValueError, match='push after flush'):
        fs.push(torch.zeros(2, 10, device=DEV))
    with pytest.raises(ValueError, match='flush called twice'):
        fs.flush()
    fs.reset()
    for bad, what in ((torch.zeros(2, 10), 'float32 on'), (torch.zeros(3, 10, device=DEV), 'expected a'), (torch.zeros(2, 10, 1, device=DEV), 'expected a'),
                      (torch.zeros(2, 10, device=DEV, dtype=torch.float64), 'float32 on')):
        with pytest.raises(ValueError, match=what):
            fs.push(bad)
    m = build(cases.ARCH_A, 'lively')
    sess = m.stream(batch=2, max_chunk=32, frontend=fe)
    with torch.no_grad():
        with pytest.raises(ValueError, match='expected a'):
            sess.push_audio(torch.zeros(2, 100))
        with pytest.raises(ValueError, match='expected a'):
            sess.push_audio(torch.zeros(1, 100, device=DEV))
        assert sess.push_audio(w[:, :100]).shape == (2, 0, 49)
        with pytest.raises(ValueError, match='push after push_audio'):
            sess.push(torch.zeros(2, 80, 4, device=DEV))
        with pytest.raises(ValueError, match='more than 200 samples'):
            sess.flush()
        sess.push_audio(w[:, 100:400])
        assert sess.flush().shape == (2, hip.output_frames(3), 49)
        with pytest.raises(ValueError, match='reset'):
            sess.push_audio(torch.zeros(2, 100, device=DEV))
        sess.reset()
        sess.push(torch.zeros(2, 80, 4, device=DEV))
        with pytest.raises(ValueError, match='push_audio after push'):
            sess.push_audio(torch.zeros(2, 100, device=DEV))
        with pytest.raises(ValueError, match='front-end'):
            m.stream(batch=2).push_audio(torch.zeros(2, 100, device=DEV))


def test_reset_starts_a_fresh_stream():
    mean, var = stats()
    fe = frontend.LogMelFrontend(mean=mean, variance=var, device=DEV)
    a = torch.stack([keyed_wave(100 + i, 5000) for i in range(2)]).to(DEV)
    c = torch.stack([keyed_wave(110 + i, 3333) for i in range(2)]).to(DEV)
    fs = fe.stream(2)
    streamed(fs, a, sizes_of(400, 5000))
    fs.reset()
    again = torch.cat(streamed(fs, c, sizes_of('ragged', 3333)), 2)
    fresh = torch.cat(streamed(fe.stream(2), c, sizes_of('ragged', 3333)), 2)
    assert torch.equal(again, fresh)
    m = build(cases.ARCH_A, 'lively')
    sess = m.stream(batch=2, max_chunk=32, frontend=fe)
    with torch.no_grad():
        run = lambda s, w: torch.cat([s.push_audio(w[:, :2000]), s.push_audio(w[:, 2000:]), s.flush()], 1)
        run(sess, a)
        sess.reset()
        assert torch.equal(run(sess, c), run(m.stream(batch=2, max_chunk=32, frontend=fe), c))
