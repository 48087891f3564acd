"""bfloat16 streaming sessions on the device (``StreamingSession(model16, batch, dtype=torch.bfloat16)``): the window kernel
nbasr_stream_window_bf16 against torch slicing, bit for bit; streamed bfloat16 logits against the golden fixtures of the bf16 path by the
rule of test_model_gpu.py::test_model_bf16_golden; every chunking the same bits; peek, waveform input, decoding and the listeners, memory,
refusals and interleaving with ``model16(x)``."""
import functools
import itertools

import numpy as np
import pytest
import torch

import cases
import nb_asr_amd as nb
from nb_asr_amd import ctc, frontend, hip, streaming
from nb_asr_amd.weights import keyed_fill_, keyed_input
from test_streaming_gpu import chunk_sizes

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
BF16 = torch.bfloat16
KINDS = [1, 7, 64, 160, 'ragged', 'whole']
CASES = {c[0]: c for c in cases.BF16_CASES}


@pytest.fixture(scope='module')
def bf16_fx():
    from conftest import GOLDEN
    with np.load(GOLDEN / 'bf16_fixtures.npz') as z:
        return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def model_of(tag):
    _, arch, use_rnn, mode, _, _ = CASES[tag]
    m = nb.get_model(arch, use_rnn=use_rnn, dropout_rate=0.0)
    keyed_fill_(m, seed=1235, mode=mode)                      # fp32 fill, THEN the cast: what the fixture generator did
    return m.to(DEV).to(BF16).eval()


def input_of(tag):
    return keyed_input(CASES[tag][4], CASES[tag][5], seed=0).to(BF16).to(DEV)


def session(tag, **kw):
    return streaming.StreamingSession(model_of(tag), CASES[tag][4], dtype=BF16, **kw)


def feed(sess, x, sizes, decode=False):
    """[result of every push, then of the flush] of x cut into ``sizes``."""
    outs, at = [], 0
    with torch.no_grad():
        for n in sizes:
            outs.append(sess.push(x[:, :, at:at + n], decode=decode))
            at += n
        outs.append(sess.flush(decode=decode))
    assert at == x.shape[2]
    return outs


@functools.lru_cache(maxsize=None)
def streamed(tag, kind):
    """(streamed logits of the case under one chunking, the session's frames_out): computed once, shared, never written to."""
    x = input_of(tag)
    sess = session(tag)
    outs = feed(sess, x, chunk_sizes(kind, x.shape[2]))
    return torch.cat(outs, 1), sess.frames_out


def same(a, b):
    """Results of push / flush / peek, tensors and nested sequences of them, bit for bit."""
    if isinstance(a, torch.Tensor):
        return isinstance(b, torch.Tensor) and a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.cpu(), b.cpu())
    if isinstance(a, (tuple, list)):
        return isinstance(b, (tuple, list)) and len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    return a == b


def bits(t):
    return t.contiguous().view(torch.int16)


# ---- the kernel ----------------------------------------------------------------------------------------------------------------------
def bf16_noise(gen, shape):
    """Every bit pattern can come up: infinities, subnormals and NaNs with their payloads included."""
    return torch.randint(-32768, 32768, shape, generator=gen, dtype=torch.int32).to(torch.int16).view(BF16)


def padded(values, off, extra):
    """``values`` (rows, n) inside rows of NaN: ``off`` unused columns in front, ``extra`` behind."""
    rows, n = values.shape
    full = torch.full((rows, off + n + extra), float('nan'), dtype=values.dtype)
    full[:, off:off + n] = values
    return full


@pytest.mark.parametrize('src_dtype', [BF16, torch.float32])
def test_window_kernel_equals_torch_slicing(src_dtype):
    gen = torch.Generator().manual_seed(20)
    offsets = list(zip((0, 1, 7, 8, 9), (9, 0, 1, 7, 8))) + [(0, 0), (8, 8)]          # (hist_off, src_off): every value of both
    exact = 0
    for rows, dst_ld, (hist_off, src_off), n_hist, n_new in itertools.product((1, 3, 5), (8, 16, 72, 136), offsets, (0, 1, 7, 8, 15), (0, 1, 8, 13)):
        if n_hist + n_new > dst_ld:
            continue
        exact += n_hist + n_new == dst_ld
        hist = bf16_noise(gen, (rows, n_hist))
        new = bf16_noise(gen, (rows, n_new)) if src_dtype == BF16 else torch.randn(rows, n_new, generator=gen) * 3.0
        want = torch.zeros(rows, dst_ld, dtype=torch.int16)     # (as bits: nothing may quieten a NaN on the way)
        want[:, :n_hist] = bits(hist)
        want[:, n_hist:n_hist + n_new] = bits(new.to(BF16))
        h = padded(hist, hist_off, 3).to(DEV)[None]
        s = padded(new, src_off, 2).to(DEV)[None]
        dst = torch.full((1, rows, dst_ld), 0x7FFF, dtype=torch.int16, device=DEV).view(BF16)
        hip.stream_window_bf16(h if n_hist else None, hist_off, n_hist, s if n_new else None, src_off, n_new, dst)
        assert torch.equal(bits(dst[0]).cpu(), want), (rows, dst_ld, hist_off, src_off, n_hist, n_new)
    assert exact >= 20                                          # n_hist + n_new == dst_ld was among them
    # batch > 1: row r of utterance r / channels, windows with their own pitches
    hist, new = bf16_noise(gen, (6, 11)), (bf16_noise(gen, (6, 5)) if src_dtype == BF16 else torch.randn(6, 5, generator=gen))
    dst = torch.full((2, 3, 24), 0x7FFF, dtype=torch.int16, device=DEV).view(BF16)
    hip.stream_window_bf16(padded(hist, 2, 1).view(2, 3, 14).to(DEV), 2, 11, padded(new, 3, 0).view(2, 3, 8).to(DEV), 3, 5, dst)
    got = bits(dst).cpu().view(6, 24)
    assert torch.equal(got[:, :11], bits(hist)) and torch.equal(got[:, 11:16], bits(new.to(BF16))) and not got[:, 16:].any()


def test_window_kernel_rounds_fp32_frames_as_torch_does():
    words = [0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x00000001, 0x80000001, 0x00012345, 0x007FFFFF, 0x00008000, 0x00018000,
             0x3F808000, 0x3F818000, 0x3F800001, 0x3F807FFF, 0x3F808001, 0xBF808000, 0xBF818000, 0x7F7F0000, 0x7F7F8000, 0x3DCCCCCD]
    src = torch.from_numpy(np.concatenate([np.array(words, np.uint32).view(np.float32), np.array([3.4e38, -3.4e38, np.nan], np.float32),
                                           np.array([0x7FA00001], np.uint32).view(np.float32)]))          # (a signalling NaN with a payload)
    nan_at = torch.isnan(src)
    assert int(nan_at.sum()) == 2
    n = src.numel()
    dst = torch.full((1, 1, 24), 0x7FFF, dtype=torch.int16, device=DEV).view(BF16)
    hip.stream_window_bf16(None, 0, 0, padded(src[None], 5, 1).to(DEV)[None], 5, n, dst)
    got, want = dst[0, 0].cpu(), src.to(BF16)
    assert torch.equal(bits(got[:n])[~nan_at], bits(want)[~nan_at]) and torch.isnan(got[:n][nan_at]).all()
    find = lambda word: bits(got)[words.index(word)].item() & 0xFFFF
    assert find(0x3F808000) == 0x3F80 and find(0x3F818000) == 0x3F82                   # ties go to the even neighbour
    assert find(0x80000000) == 0x8000 and find(0x00008000) == 0x0000 and find(0x00018000) == 0x0002      # -0; subnormal ties
    assert torch.isinf(got[len(words)]) and torch.isinf(got[len(words) + 1]) and got[len(words) + 1] < 0  # 3.4e38 rounds to inf
    # bfloat16 sources: the bits, NaN payloads included
    pay = torch.from_numpy(np.array([0x7FC1, 0x7F81, 0xFFFF, 0x7F80, 0x0001, 0x8000, 0x7FFF, 0x1234], np.uint16).view(np.int16))
    dst = torch.zeros((1, 1, 8), dtype=BF16, device=DEV)
    hip.stream_window_bf16(None, 0, 0, pay.view(BF16).view(1, 1, 8).to(DEV), 0, 8, dst)
    assert torch.equal(bits(dst).cpu().flatten(), pay)


# ---- the session against the golden fixtures, and against itself ---------------------------------------------------------------------
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('tag', list(CASES))
def test_streamed_logits_meet_the_golden_rule_of_the_bf16_path(bf16_fx, tag, kind):
    logits, frames_out = streamed(tag, kind)
    ref, truth = torch.from_numpy(bf16_fx[f'{tag}/logits']).double(), torch.from_numpy(bf16_fx[f'{tag}/logits_f64'])
    assert logits.dtype == BF16 and tuple(logits.shape) == tuple(ref.shape) and torch.isfinite(logits).all()
    assert frames_out == hip.output_frames(CASES[tag][5]) == ref.shape[1]
    got = logits.double().cpu()
    e_ref, e_hip = cases._rms(ref - truth), cases._rms(got - truth)
    m_ref, m_hip = float((ref - truth).abs().max()), float((got - truth).abs().max())
    print(f'{tag} chunks {kind}: logits rms err vs fp64: streamed {e_hip:.3e}, reference bf16 {e_ref:.3e}; max: streamed {m_hip:.3e}, reference {m_ref:.3e}')
    assert e_hip <= 1.25 * e_ref
    assert m_hip <= 1.5 * m_ref


@pytest.mark.parametrize('tag', list(CASES))
def test_chunking_changes_nothing(tag):
    whole, _ = streamed(tag, 'whole')
    for kind in KINDS:
        assert torch.equal(streamed(tag, kind)[0], whole), (tag, kind)


def test_against_the_whole_forward():
    """Every LayerNorm sits where ``walk.WalkBf16`` puts it, so a session can differ from ``model16(x)`` only where the whole forward
    takes a cell LayerNorm's statistics from the producing node launch's epilogue (cells that are not conv-only, ending in a grouped
    conv, in front of a consumer that normalises on load) while the session takes them from a pass over the stored rows.  Measured on
    an MI355X (DESIGN.md 9 "bf16 sessions"): D_lively_b2_t200 0 of 4 900 logits differ, D_xavier_b1_t131 0 of 1 617, A_lively_b1_t160 0
    of 1 960; Z_lively_b2_t90_nornn 2 081 of 2 254, largest difference 1.56e-1, first at the second cell of block 0 -- there the golden
    rule above is the gate."""
    from nb_asr_amd.ops import PadConvRelu
    from nb_asr_amd.walk import cheap_consumer
    for tag in CASES:
        m, x = model_of(tag), input_of(tag)
        with torch.no_grad():
            want = m(x)
        got = streamed(tag, 'whole')[0]
        differing = int((bits(got) != bits(want)).sum())
        print(f'{tag}: {differing} of {got.numel()} logits differ from model16(x), largest difference {float((got.float() - want.float()).abs().max()):.3e}')
        cell, last = m.model[2], m.model[2].nodes[-1].op
        by_product = (not session(tag)._stages.cell_mfma and cell.use_norm and cheap_consumer(cell) and isinstance(last, PadConvRelu) and last.groups > 1)
        assert got.shape == want.shape and got.dtype == want.dtype
        assert by_product or torch.equal(got, want), tag
    assert session('D_lively_b2_t200')._stages.cell_mfma                   # (the conv-only cases do run the matrix-core cell)


# ---- peek ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tag', ['D_xavier_b1_t131', 'Z_lively_b2_t90_nornn'])
def test_peek_is_the_flush_of_a_twin_and_leaves_the_session_alone(tag):
    x = input_of(tag)
    t = x.shape[2]
    sizes = [40, 23, 1, t - 64]
    peeker, never = session(tag, max_chunk=32), session(tag, max_chunk=32)
    at = 0
    with torch.no_grad():
        for i, n in enumerate(sizes):
            piece = x[:, :, at:at + n]
            at += n
            assert same(peeker.push(piece, decode='beam'), never.push(piece, decode='beam'))
            if i == 0 or i == 2:
                twin = session(tag, max_chunk=32)
                feed_at = 0
                for m in sizes[:i + 1]:
                    twin.push(x[:, :, feed_at:feed_at + m], decode='beam')
                    feed_at += m
                want = twin.flush(decode='beam')
                plain, beamed = peeker.peek(), peeker.peek(decode='beam')
                assert plain.dtype == BF16 and plain.shape[1] > 0
                assert same(plain, want[0]) and same(beamed, want)
        assert same(peeker.flush(decode='beam'), never.flush(decode='beam'))


# ---- the waveform --------------------------------------------------------------------------------------------------------------------
def wave(batch, samples, seed):
    gen = torch.Generator().manual_seed(seed)
    t = torch.arange(samples) / 16000.0
    tone = 0.3 * torch.sin(2 * torch.pi * 440.0 * t) + 0.2 * torch.sin(2 * torch.pi * 3100.0 * t)
    return (tone[None] + 0.1 * torch.randn(batch, samples, generator=gen)).to(DEV)


@pytest.mark.parametrize('rate', [None, 8000])
def test_push_audio_is_push_of_the_rounded_frames(rate):
    tag = 'D_xavier_b1_t131'
    fe = frontend.LogMelFrontend(device=DEV)
    samples = 8000 if rate is None else 4000                     # half a second
    w = wave(1, samples, 7)
    sizes = [1600, 37, 0, 3000, 213, 3150] if rate is None else [800, 37, 0, 1500, 213, 1450]
    assert sum(sizes) == samples
    audio = session(tag, max_chunk=64, frontend=fe, input_rate=rate)
    plain = session(tag, max_chunk=64)
    fs = fe.stream(1)
    rs = frontend.Resampler(rate, 16000, device=DEV).stream(1) if rate else None
    got, want, at = [], [], 0
    with torch.no_grad():
        for n in sizes:
            piece = w[:, at:at + n]
            at += n
            got.append(audio.push_audio(piece))
            want.append(plain.push(fs.push(rs.push(piece) if rs else piece).to(BF16)))
        got.append(audio.flush())
        if rs:
            want.append(plain.push(fs.push(rs.flush()).to(BF16)))
        want.append(plain.push(fs.flush().to(BF16)))
        want.append(plain.flush())
    for g, p in zip(got[:-1], want):                             # push by push
        assert g.dtype == BF16 and same(g, p)
    g, p = torch.cat(got, 1), torch.cat(want, 1)
    assert g.shape[1] == audio.frames_out == plain.frames_out > 0 and torch.equal(g, p)


# ---- decoding and the listeners read logits.float() ----------------------------------------------------------------------------------
def test_decodes_and_listeners_are_the_offline_functions_on_the_widened_logits():
    tag = 'D_lively_b2_t200'
    x, b = input_of(tag), CASES[tag][4]
    sizes = [50, 1, 0, 70, 7, 72]
    outs = feed(session(tag, max_chunk=64), x, sizes, decode=True)
    logits = torch.cat([o[0] for o in outs], 1)
    assert logits.dtype == BF16 and torch.equal(logits, streamed(tag, 'whole')[0])
    tokens = [[t for o in outs for t in o[1][i].tolist()] for i in range(b)]
    assert [w.tolist() for w in ctc.greedy_decode(logits.float())] == tokens
    outs = feed(session(tag, max_chunk=64), x, sizes, decode='beam')
    assert torch.equal(torch.cat([o[0] for o in outs], 1), logits)
    assert same(outs[-1][1], ctc.beam_decode(ctc.log_softmax(logits.float()), None, 12, 0, 40))
    rules, conf = ctc.EndpointRules(rules=((0, 12, 0), (1, 3, 0), (0, 0, 40))), ctc.ConfidenceRules()
    sess = session(tag, max_chunk=64, endpoint=rules, confidence=conf)
    assert torch.equal(torch.cat(feed(sess, x, sizes), 1), logits)
    assert torch.equal(sess.endpoint.state, ctc.endpoint(logits.float(), None, rules).state)
    assert torch.equal(sess.confidence.last.state, ctc.confidence(logits.float(), None, conf).state)


# ---- memory --------------------------------------------------------------------------------------------------------------------------
def test_memory_is_below_the_float32_sessions_and_bounded():
    tag = 'D_xavier_b1_t131'
    _, arch, use_rnn, mode, _, _ = CASES[tag]
    m32 = nb.get_model(arch, use_rnn=use_rnn, dropout_rate=0.0)
    keyed_fill_(m32, seed=1235, mode=mode)
    m32 = m32.to(DEV).eval()
    sess16, sess32 = session(tag, max_chunk=40), m32.stream(batch=1, max_chunk=40)
    print(f'buffer_bytes: bfloat16 session {sess16.buffer_bytes}, float32 session {sess32.buffer_bytes}')
    assert sess16.buffer_bytes < sess32.buffer_bytes
    del sess32, m32
    x = keyed_input(1, 1200, seed=5).to(BF16).to(DEV)
    marks = {}
    with torch.no_grad():
        for i in range(30):
            sess16.push(x[:, :, 40 * i:40 * i + 40])
            if i + 1 in (10, 30):
                torch.cuda.synchronize()
                marks[i + 1] = torch.cuda.memory_allocated()
    assert marks[10] == marks[30]


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    tag = 'A_lively_b1_t160'
    m16 = model_of(tag)
    _, arch, use_rnn, mode, _, _ = CASES[tag]
    m32 = nb.get_model(arch, use_rnn=use_rnn, dropout_rate=0.0).to(DEV).eval()
    with pytest.raises(ValueError, match='does not match'):
        streaming.StreamingSession(m32, 1, dtype=BF16)
    with pytest.raises(ValueError, match='does not match'):
        streaming.StreamingSession(m16, 1, dtype=torch.float32)
    with pytest.raises(ValueError, match='dtype'):
        streaming.StreamingSession(m16, 1, dtype=torch.float16)
    with pytest.raises(ValueError, match='float32'):             # the untouched default
        m16.stream(batch=1)
    with pytest.raises(ValueError, match='bfloat16'):
        session(tag).push(torch.zeros(1, 80, 10, device=DEV))
    with pytest.raises(ValueError, match='float32'):
        m32.stream(batch=1).push(torch.zeros(1, 80, 10, device=DEV, dtype=BF16))
    with torch.no_grad():                                        # dtype=torch.float32 is the session without the argument
        x = keyed_input(1, 60, seed=2).to(DEV)
        a, b = streaming.StreamingSession(m32, 1, dtype=torch.float32), m32.stream(batch=1)
        assert same([a.push(x), a.flush()], [b.push(x), b.flush()])


# ---- interleaving with the whole forward ---------------------------------------------------------------------------------------------
def test_whole_forwards_in_between_disturb_nothing():
    tag = 'Z_lively_b2_t90_nornn'
    m, x = model_of(tag), input_of(tag)
    y = keyed_input(2, 77, seed=4).to(BF16).to(DEV)
    sess = session(tag)
    got, at = [], 0
    with torch.no_grad():
        first = m(y)
        for n in (30, 41, 19):
            got.append(sess.push(x[:, :, at:at + n]))
            at += n
            assert torch.equal(m(y), first)
        got.append(sess.flush())
        assert torch.equal(m(y), first)
    assert torch.equal(torch.cat(got, 1), streamed(tag, 'whole')[0])
