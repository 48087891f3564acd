"""The HIP resampler on the device: precision against the float64 definition (resample_model.py) within a derived bound, bits that do not
depend on the chunking, the batch or its padding, the stream's contract, and sessions fed samples at another rate than 16 kHz."""
import functools

import numpy as np
import pytest
import torch

import cases
import resample_model as rm
from nb_asr_amd import frontend, hip, streaming
from test_stream_launch_sequence_gpu import model_for, normalise, pushes, waves

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
PAIRS = [(8000, 16000), (11025, 16000), (22050, 16000), (44100, 16000), (48000, 16000), (16000, 8000)]


def ragged(o):
    return (1, 0, 7, o, o + 1, 3 * o, 50, 0, 2, 441, 5)


@functools.lru_cache(maxsize=None)
def resampler(orig, new):
    return frontend.Resampler(orig, new, device=DEV)


def lengths_for(o):
    """A few thousand samples just below, at and above a multiple of o, and one utterance shorter than any support."""
    k = max(1, 2400 // o) * o
    return (k - 1, k, k + 1, 5)


@functools.lru_cache(maxsize=None)
def utterance(orig, new, length):
    """(samples float32, float64 model, its bound), made once per case and never written to."""
    o, n = rm.ratio(orig, new)
    x = np.random.default_rng(orig + 7 * new + length).standard_normal(length).astype(np.float32)
    y, bound = rm.resample64(x, o, n)
    for a in (x, y, bound):
        a.setflags(write=False)
    return x, y, bound


@functools.lru_cache(maxsize=None)
def alone(orig, new, length):
    """The utterance resampled on its own, whole: what every other route must reproduce bit for bit."""
    x, _, _ = utterance(orig, new, length)
    out, out_lengths = resampler(orig, new)(torch.from_numpy(x.copy())[None].to(DEV))
    assert out_lengths == [out.shape[1]]
    return out[0].cpu()


def sizes_for(pattern, length):
    """``pattern`` repeated until ``length`` samples are cut."""
    at, i, sizes = 0, 0, []
    while at < length:
        sizes.append(min(pattern[i % len(pattern)], length - at))
        at += sizes[-1]
        i += 1
    return sizes


def streamed(rs, wave, sizes):
    """cat(pushes, flush) of ``wave`` (B, L) cut into ``sizes``; the counts after every push are the host geometry's."""
    rs.reset()
    parts, at, out = [], 0, 0
    for s in sizes:
        parts.append(rs.push(wave[:, at:at + s]))
        at, out = at + s, out + parts[-1].shape[1]
        assert parts[-1].shape[0] == wave.shape[0] and rs.samples_in == at
        assert rs.samples_out == out == frontend.resample_final(at, rs.o, rs.n)                  # (== the model's count: the host tests)
    parts.append(rs.flush())
    assert rs.samples_out == frontend.resample_total(at, rs.o, rs.n)
    return torch.cat(parts, 1).cpu()


@pytest.mark.parametrize('orig,new', PAIRS)
def test_precision_against_the_float64_definition(orig, new):
    """|got - float64| <= (taps + 2) 2^-24 sum_m |h x|: one rounding per product, one per sum, one for the float32 table."""
    o, n = rm.ratio(orig, new)
    taps = rm.largest_support(o, n)
    assert taps == resampler(orig, new).taps
    for length in lengths_for(o):
        _, y, bound = utterance(orig, new, length)
        got = alone(orig, new, length).numpy().astype(np.float64)
        assert got.shape == y.shape == (rm.total(length, o, n),)
        err, allowed = np.abs(got - y), rm.error_bound(bound, taps)
        print(f'{orig}->{new} L={length}: max err / bound = {np.max(err / np.maximum(allowed, 1e-300)):.3f}')
        assert np.all(err <= allowed)


@pytest.mark.parametrize('batch', (1, 3))
@pytest.mark.parametrize('orig,new', PAIRS)
def test_chunked_equals_whole_and_a_batch_row_equals_the_utterance_alone(orig, new, batch):
    o, n = rm.ratio(orig, new)
    length = lengths_for(o)[1 if batch == 1 else 2]              # (batch 1: a multiple of o; batch 3: one sample more)
    rows = [length + 97 * b for b in range(batch)]               # other utterances, cut to the same length: other seeds
    wave = torch.stack([torch.from_numpy(utterance(orig, new, r)[0][:length].copy()) for r in rows]).to(DEV)
    want = torch.stack([alone(orig, new, rows[0])] + [resampler(orig, new)(wave[b:b + 1])[0][0].cpu() for b in range(1, batch)])
    whole, out_lengths = resampler(orig, new)(wave)
    assert out_lengths == [rm.total(length, o, n)] * batch and torch.equal(whole.cpu(), want)
    rs = resampler(orig, new).stream(batch)
    assert rs.state_bytes == hip.resample_state_bytes(batch, resampler(orig, new).tail_capacity) > 0
    for sizes in (sizes_for((o,), length), sizes_for((160,), length), sizes_for(ragged(o), length), [length]):
        assert torch.equal(streamed(rs, wave, sizes), want), sizes[:12]
    short = wave[:, :3 * rm.largest_support(o, n)].contiguous()   # pushes of one sample, a short utterance
    assert torch.equal(streamed(rs, short, [1] * short.shape[1]), resampler(orig, new)(short)[0].cpu())


@pytest.mark.parametrize('orig,new', PAIRS)
def test_ragged_batch_with_poisoned_padding(orig, new):
    o, n = rm.ratio(orig, new)
    lengths = [lengths_for(o)[0], lengths_for(o)[2], lengths_for(o)[3]]
    wave = torch.full((3, max(lengths) + 9), float('nan'))
    for b, length in enumerate(lengths):
        wave[b, :length] = torch.from_numpy(utterance(orig, new, length)[0].copy())
    out, out_lengths = resampler(orig, new)(wave.to(DEV), lengths=lengths)
    out = out.cpu()
    assert out.shape == (3, rm.total(wave.shape[1], o, n)) and out_lengths == [rm.total(v, o, n) for v in lengths]
    assert not torch.isnan(out).any()
    for b, length in enumerate(lengths):
        assert torch.equal(out[b, :out_lengths[b]], alone(orig, new, length))
        assert not out[b, out_lengths[b]:].any()
    as_tensor, _ = resampler(orig, new)(wave.to(DEV), lengths=torch.tensor(lengths, dtype=torch.int32, device=DEV))
    assert torch.equal(as_tensor.cpu(), out)


@pytest.mark.parametrize('orig,new', [(48000, 16000), (11025, 16000), (16000, 8000)])
def test_stream_contract(orig, new):
    r = resampler(orig, new)
    o, n = r.o, r.n
    wave = torch.stack([torch.from_numpy(utterance(orig, new, lengths_for(o)[2] + 97 * b)[0][:2000].copy()) for b in range(2)]).to(DEV)
    rs, twin = r.stream(2), r.stream(2)
    sizes = sizes_for(ragged(o), 2000)
    # peek == the flush of a twin, bit for bit, at every cut (before the first sample too); the stream goes on as if never peeked
    untouched = streamed(r.stream(2), wave, sizes)
    parts, at = [], 0
    for i, s in enumerate([0] + sizes):
        parts.append(rs.push(wave[:, at:at + s]))
        at += s
        peeked = rs.peek()
        assert peeked.shape[1] == frontend.resample_peek(at, o, n) <= r.max_pending and rs.pending == peeked.shape[1]
        if i % 3 == 0 or at == 2000:
            twin.reset()
            twin.push(wave[:, :at])
            assert torch.equal(peeked, twin.flush())
    parts.append(rs.flush())
    assert torch.equal(torch.cat(parts, 1).cpu(), untouched)
    for call in (rs.flush, rs.peek, lambda: rs.push(wave[:, :4])):
        with pytest.raises(ValueError, match='reset'):
            call()
    twin.reset()
    with pytest.raises(ValueError, match='chunk'):           # the batch is lockstep
        twin.push(wave[:1, :4])
    # the state is the two tails and stays so: 200 pushes, the ABI's number
    rs.reset()
    before = rs.state_bytes
    tails = rs._tails.data_ptr()
    for i in range(200):
        rs.push(wave[:, (7 * i) % 1000:(7 * i) % 1000 + 1 + i % 9])
    assert rs.state_bytes == before == hip.resample_state_bytes(2, r.tail_capacity) == 2 * 2 * hip.round_up4(r.tail_capacity) * 4
    assert rs._tails.data_ptr() == tails and rs.lookahead_samples == frontend.resample_lookahead(o, n)


def test_refusals_on_the_device():
    r = resampler(48000, 16000)
    with pytest.raises(hip.HipError, match='HIP device'):
        r(torch.zeros(1, 100))
    with pytest.raises(ValueError, match='lengths'):
        r(torch.zeros(2, 100, device=DEV), lengths=[50, 101])
    tails = torch.zeros(2, 1, 36, device=DEV)
    out = torch.zeros(1, 64, device=DEV)
    wave = torch.zeros(1, 100, device=DEV)
    with pytest.raises(hip.HipError, match='need samples'):            # output 28 needs samples beyond the 100 held
        hip.resample_stream_step(tails[0], 0, 0, wave, tails[1], 0, 36, r.table(), 48000, 16000, out, 0, 0, 29, False)
    with pytest.raises(hip.HipError, match='in turn'):
        hip.resample_stream_step(tails[0], 0, 0, wave, tails[0], 70, 36, r.table(), 48000, 16000, out, 0, 0, 28, False)
    with pytest.raises(hip.HipError, match='16-byte'):
        odd = torch.zeros(40, device=DEV)[1:37].view(1, 36)             # 4 bytes past a 16-byte boundary
        hip.resample_stream_step(tails[0], 0, 0, wave, odd, 70, 36, r.table(), 48000, 16000, out, 0, 0, 28, False)


# ---- sessions ------------------------------------------------------------------------------------------------------------------
def front_end():
    return frontend.LogMelFrontend(device=DEV)


def session(rate, fe, max_chunk=64):
    return streaming.StreamingSession(model_for(cases.ARCH_M, True), 2, max_chunk, 4, frontend=fe, input_rate=rate)


def same(a, b):
    """Results of push / flush / peek, tensors and nested sequences of them, bit for bit."""
    if isinstance(a, torch.Tensor):
        return isinstance(b, torch.Tensor) and a.shape == b.shape and torch.equal(a.cpu(), b.cpu())
    if isinstance(a, (tuple, list)):
        return isinstance(b, (tuple, list)) and len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    return a == b


@pytest.mark.parametrize('rate', (48000, 8000))
def test_session_at_another_rate_is_the_16k_session_on_the_resampled_waveform(rate):
    """push_audio in chunks at ``rate`` then flush == a 16 kHz session fed Resampler(rate)(whole waveform), cut where the stream's
    pushes released their outputs (a session's steps, and with them the f16x2 window scales, follow the frames a push completes)."""
    r = resampler(rate, 16000)
    fe = front_end()
    wave = waves(2, rate // 2 + 37, 40)                          # half a second: about 50 frames
    whole, _ = r(wave)
    sizes = sizes_for((3 * rate // 16, 0, rate // 10 + 11, 1), wave.shape[1])
    cuts = np.cumsum(sizes)
    resampled, plain = session(rate, fe), session(None, fe)
    assert resampled.lookahead_samples == -(-plain.lookahead_samples * r.o // r.n) + r.lookahead_samples
    assert resampled.buffer_bytes == plain.buffer_bytes + r.stream(2).state_bytes and resampled.end_frames == 2
    with torch.no_grad():
        for decode in (True, 'beam'):
            resampled.reset(), plain.reset()
            at = done = 0
            for s, cut in zip(sizes, cuts):
                got = resampled.push_audio(wave[:, at:at + s], decode=decode)
                final = frontend.resample_final(int(cut), r.o, r.n)
                want = plain.push_audio(whole[:, done:final], decode=decode)
                assert same(got, want), (decode, at)
                at, done = at + s, final
            plain.push_audio(whole[:, done:], decode=decode)     # (the resampler's flush: its last outputs as a push)
            got, want = resampled.flush(decode=decode), plain.flush(decode=decode)
            assert got[0].shape[1] > 0 and same(got[0], want[0]) and same(got[1], want[1])
    with pytest.raises(ValueError, match='max_chunk=1 is below'):
        session(rate, fe, max_chunk=1)
    with pytest.raises(ValueError, match='front-end'):
        streaming.StreamingSession(model_for(cases.ARCH_M, True), 2, 64, input_rate=rate)


def test_session_peek_is_the_flush_of_a_twin():
    """At 48 kHz, with a peek before any frame is out: 618 samples give 200 final outputs and 6 pending, so the end carries the
    front-end past its 200 samples.  After 5881 samples 1955 outputs are final and frame 11 waits for 5 more: the 6 pending outputs
    complete it, so that peek too takes two steps ahead of the final one, now on windows with history.  The peeked session then goes
    on as one that never peeked."""
    rate, fe = 48000, front_end()
    wave = waves(2, 19000, 50)
    sizes = (300, 318, 5263, 0, 13119)
    assert frontend.frames_final(1955 + 6) - frontend.frames_final(1955) == 1 == frontend.resample_final(5881, 3, 1) - 1954
    sess, twin = session(rate, fe), session(rate, fe)
    with torch.no_grad():
        for decode in (True, 'beam'):
            sess.reset()
            pushed, peeked, at = [], [], 0
            assert sess.peek(decode=decode)[0].shape[1] == 0
            for s in sizes:
                pushed.append(sess.push_audio(wave[:, at:at + s], decode=decode))
                at += s
                peeked.append(sess.peek(decode=decode))
            last = sess.flush(decode=decode)
            assert peeked[0][0].shape[1] == 0 and peeked[1][0].shape[1] > 0 and pushed[1][0].shape[1] == 0      # 300: nothing; 618: a peek ahead of every frame
            for upto in (2, 3, 5):                               # the twin: the same pushes, then the end
                twin.reset()
                at, outs = 0, []
                for s in sizes[:upto]:
                    outs.append(twin.push_audio(wave[:, at:at + s], decode=decode))
                    at += s
                flushed = twin.flush(decode=decode)
                assert same(peeked[upto - 1], flushed), (decode, upto)
                assert all(same(a, b) for a, b in zip(pushed, outs))
            assert same(last, flushed)


def test_input_rate_16000_is_the_session_without_the_argument_launch_for_launch():
    fe = front_end()
    wave = waves(2, 12801, 60)
    listings = []
    for rate in (None, 16000):
        sess = session(rate, fe)
        assert sess._resampler is None
        script = lambda: pushes(sess, wave, (8000, 4801, 0), True, audio=True)
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
        listings.append(normalise(sess, entries))
    assert len(listings[0]) > 50 and listings[0] == listings[1]
    assert not any('resample' in line for line in listings[0])
