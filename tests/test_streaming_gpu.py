"""Streaming inference on the device (nb_asr_amd/streaming.py): chunk-by-chunk pushes with carried state give the whole forward's logits
(the parity rule of tests/cases.py against the golden fixtures and against model(x)), emit exactly the frames the planner predicts, keep
their memory bounded, carry the LSTM state through nbasr_lstm_recurrence_frames16_state and decode greedily across push boundaries."""
import pytest
import torch

import cases
import nb_asr_amd as nb
from nb_asr_amd import hip, streaming
from nb_asr_amd.weights import keyed_fill_, keyed_input

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def build(arch, use_rnn, mode, seed=1235):
    m = nb.get_model(arch, use_rnn=use_rnn, dropout_rate=0.0)
    keyed_fill_(m, seed=seed, mode=mode)
    return m.to(DEV).eval()


def chunk_sizes(kind, t):
    if kind == 'whole':
        return [t]
    if kind == 'ragged':
        sizes, i = [], 0
        pattern = (3, 0, 41, 200, 1, 17, 96, 5)
        while sum(sizes) < t:
            sizes.append(min(pattern[i % len(pattern)], t - sum(sizes)))
            i += 1
        return sizes
    return [min(kind, t - i) for i in range(0, t, kind)]


def stream(model, x, sizes, max_chunk=160, sess=None):
    """Streamed logits of x cut into ``sizes``: (concatenated logits, per-push frame counts, session)."""
    sess = sess or model.stream(batch=x.shape[0], max_chunk=max_chunk)
    outs, at = [], 0
    with torch.no_grad():
        for n in sizes:
            outs.append(sess.push(x[:, :, at:at + n]))
            at += n
        outs.append(sess.flush())
    assert at == x.shape[2]
    return torch.cat(outs, 1), [o.shape[1] for o in outs], sess


def planner_counts(sess, sizes, max_chunk):
    """Per-push emitted frames the planner predicts (pushes larger than max_chunk split like the session splits them)."""
    p = streaming.StreamPlanner(sess.specs)
    counts = []
    for n in sizes:
        got = 0
        for off in range(0, max(n, 1), max_chunk):
            plans = p.step(min(max_chunk, n - off))
            if plans[-1] is not None:
                got += plans[-1].d - plans[-1].c
        counts.append(got)
    plans = p.step(0, final=True)
    counts.append(plans[-1].d - plans[-1].c if plans[-1] is not None else 0)
    return counts


@pytest.mark.parametrize('kind', [1, 7, 64, 160, 'ragged', 'whole'])
@pytest.mark.parametrize('tag,arch,use_rnn,mode,b,t', cases.MODEL_CASES)
def test_streamed_logits_match_the_golden_fixtures(model_fx, tag, arch, use_rnn, mode, b, t, kind):
    m = build(arch, use_rnn, mode)
    x = keyed_input(b, t, seed=0).to(DEV)
    got, counts, sess = stream(m, x, chunk_sizes(kind, t))
    want = torch.from_numpy(model_fx[f'{tag}/logits'])
    assert tuple(got.shape) == tuple(want.shape) and sess.frames_out == hip.output_frames(t) == want.shape[1]
    assert torch.isfinite(got).all()
    cases.assert_parity(got, want, torch.from_numpy(model_fx[f'{tag}/logits_f64']), f'{tag} chunks {kind}')


@pytest.mark.parametrize('arch,use_rnn,mode,b,t,sizes', [
    (cases.ARCH_D, True, 'xavier', 8, 1000, [160] * 6 + [40]),
    (cases.ARCH_D, True, 'xavier', 8, 1000, [333, 0, 500, 167]),
    (cases.ARCH_M, True, 'lively', 2, 3000, [400] * 7 + [200]),
    (cases.ARCH_A, False, 'lively', 2, 3000, [1000, 2000]),
])
def test_streamed_logits_match_the_whole_forward(arch, use_rnn, mode, b, t, sizes):
    m = build(arch, use_rnn, mode)
    x = keyed_input(b, t, seed=3).to(DEV)
    with torch.no_grad():
        whole = m(x).cpu()
    got, counts, sess = stream(m, x, sizes)
    assert counts == planner_counts(sess, sizes, 160)
    assert sum(counts) == hip.output_frames(t) and tuple(got.shape) == tuple(whole.shape)
    # the whole forward as the reference, its distance to the fp64 oracle as the noise floor
    from oracle import asr_oracle as oracle
    truth = oracle.asr_forward(dict(m.state_dict()), arch, x.cpu(), use_rnn=use_rnn, dtype=torch.float64)
    cases.assert_parity(got, whole, truth, f'B={b} T={t}')


def test_session_memory_is_bounded():
    """Buffers are allocated when the session is made: the device memory in use after 10 and after 60 pushes of 400 frames is the same,
    and the streamed logits of the 24 000 frames are in parity with model(x)."""
    m = build(cases.ARCH_D, True, 'lively')
    sess = m.stream(batch=2, max_chunk=400)
    x = keyed_input(2, 400 * 60, seed=5).to(DEV)
    outs = []
    with torch.no_grad():
        for i in range(60):
            outs.append(sess.push(x[:, :, i * 400:(i + 1) * 400]).cpu())
            if i == 9:
                torch.cuda.synchronize()
                at10 = (sess.buffer_bytes, torch.cuda.memory_allocated(DEV))
        torch.cuda.synchronize()
        at60 = (sess.buffer_bytes, torch.cuda.memory_allocated(DEV))
        outs.append(sess.flush().cpu())
        whole = m(x).cpu()
    assert at10 == at60
    got = torch.cat(outs, 1)
    assert got.shape == whole.shape
    assert cases.worst_ratio(got, whole, 1e-4, 1e-5) <= 1.0


def _rand_state_case(b, t, h, seed):
    torch.manual_seed(seed)
    gates = torch.randn(t, b, 4 * h, device=DEV)
    w_hh = torch.randn(4 * h, h, device=DEV) * 0.1
    return gates, w_hh


@pytest.mark.parametrize('b,t,h', [(3, 7, 500), (17, 5, 36), (64, 30, 500), (1, 1, 500)])
def test_lstm_state_entry_without_flags_is_the_per_frame_form(b, t, h):
    gates, w_hh = _rand_state_case(b, t, h, h + b)
    packed = hip.lstm_pack_whh16(w_hh)
    ws = hip.lstm_xcd_workspace(b, h, DEV)
    cell0, out0 = torch.empty(b, h, device=DEV), torch.empty(b, t, h, device=DEV)
    hip.lstm_recurrence_frames16(gates, packed, cell0, out0, ws)
    for rep in range(4):                                      # (the third call replays the cached chain)
        cell, out = torch.full((b, h), float('nan'), device=DEV), torch.full((b, t, h), float('nan'), device=DEV)
        hip.lstm_recurrence_frames16_state(gates, packed, cell, out, ws, None, 0)
        assert torch.equal(out, out0) and torch.equal(cell, cell0), rep


@pytest.mark.parametrize('b,t,h', [(3, 30, 500), (17, 12, 36), (64, 24, 500)])
def test_lstm_state_carried_across_calls(b, t, h):
    from test_lstm_xcd_gpu import ref64
    gates, w_hh = _rand_state_case(b, t, h, 7 * h + b)
    want, c_want = ref64(gates, w_hh)
    packed = hip.lstm_pack_whh16(w_hh)
    ws = hip.lstm_xcd_workspace(b, h, DEV)
    cell, one = torch.empty(b, h, device=DEV), torch.empty(b, t, h, device=DEV)
    hip.lstm_recurrence_frames16(gates, packed, cell, one, ws)
    e_one = float((one.double().cpu() - want).abs().max())
    for split in (1, t // 3, t - 1):
        for rep in range(4):                                  # (cached chains: h0 and the flag are part of their key)
            c_state, h0 = torch.empty(b, h, device=DEV), torch.empty(b, h, device=DEV)
            parts = []
            for lo, hi in ((0, split), (split, t)):
                out = torch.empty(b, hi - lo, h, device=DEV)
                first = lo == 0
                hip.lstm_recurrence_frames16_state(gates[lo:hi].contiguous(), packed, c_state, out, ws, None if first else h0,
                                                   0 if first else hip.LSTM_CONTINUE)
                h0.copy_(out[:, -1])
                parts.append(out)
            got = torch.cat(parts, 1)
            e_split = float((got.double().cpu() - want).abs().max())
            ec = float((c_state.double().cpu() - c_want).abs().max())
            assert torch.isfinite(got).all()
            assert e_split <= 2.0 * e_one + 2e-7, (split, rep, e_split, e_one)
            assert ec <= 4e-6 * (1 + float(c_want.abs().max())), (split, rep, ec)


def test_lstm_state_entry_refuses_bad_flags():
    lib = hip.load_library()
    assert lib.nbasr_lstm_recurrence_frames16_state(16, 16, 16, 16, 16, None, 1, 1, 500, 4, None) == -1
    assert b'flags' in lib.nbasr_last_error()
    assert lib.nbasr_lstm_recurrence_frames16_state(16, 16, 16, 16, 16, 16, 1, 1, 500, 0, None) == -1
    assert b'CONTINUE' in lib.nbasr_last_error()


def test_streaming_greedy_decode_matches_the_whole_decode():
    m = build(cases.ARCH_A, True, 'lively')
    x = keyed_input(3, 700, seed=9).to(DEV)
    sess = m.stream(batch=3, max_chunk=64)
    logits, tokens = [], [[] for _ in range(3)]
    at = 0
    with torch.no_grad():
        for n in (50, 1, 0, 130, 7, 300, 212):
            lg, tk = sess.push(x[:, :, at:at + n], decode=True)
            at += n
            logits.append(lg)
            for i in range(3):
                tokens[i] += tk[i].tolist()
        lg, tk = sess.flush(decode=True)
        logits.append(lg)
        for i in range(3):
            tokens[i] += tk[i].tolist()
    want = nb.ctc.greedy_decode(torch.cat(logits, 1))
    assert [w.tolist() for w in want] == tokens


def test_streaming_greedy_collapses_a_run_across_the_boundary():
    """Logits whose argmax is one label over a run that a push boundary cuts: one token, not two."""
    b, c = 2, 49
    lg = torch.full((b, 12, c), -5.0, device=DEV)
    labels = [[0, 3, 3, 3, 3, 0, 7, 7, 0, 0, 7, 2], [5, 5, 5, 5, 5, 5, 0, 5, 5, 1, 1, 1]]
    for i in range(b):
        for t, k in enumerate(labels[i]):
            lg[i, t, k] = 4.0
    want = nb.ctc.greedy_decode(lg)
    prev = torch.full((b,), -1, dtype=torch.int32, device=DEV)
    got = [[] for _ in range(b)]
    for lo, hi in ((0, 2), (2, 2), (2, 4), (4, 7), (7, 8), (8, 12)):
        tokens, counts = hip.ctc_greedy_stream(lg[:, lo:hi].contiguous(), prev)
        for i in range(b):
            got[i] += tokens[i, : int(counts[i])].tolist()
    assert got == [w.tolist() for w in want] == [[3, 7, 7, 2], [5, 5, 1]]


def test_refusals():
    m = build(cases.ARCH_D, True, 'lively')
    with pytest.raises(ValueError, match='float32'):
        build(cases.ARCH_A, True, 'lively').to(torch.bfloat16).stream(batch=1)
    mt = nb.get_model(cases.ARCH_A, use_rnn=True, dropout_rate=0.1).to(DEV)
    with pytest.raises(ValueError, match='dropout'):
        mt.stream(batch=1)
    sess = m.stream(batch=2, max_chunk=32)
    with pytest.raises(ValueError, match='chunk'):
        sess.push(torch.zeros(3, 80, 10, device=DEV))
    with pytest.raises(ValueError, match='chunk'):
        sess.push(torch.zeros(2, 40, 10, device=DEV))
    with pytest.raises(ValueError, match='float32'):
        sess.push(torch.zeros(2, 80, 10))
    with torch.no_grad():
        sess.push(torch.zeros(2, 80, 10, device=DEV))
        sess.flush()
    with pytest.raises(ValueError, match='reset'):
        sess.push(torch.zeros(2, 80, 10, device=DEV))
    sess.reset()
    with torch.no_grad():
        sess.push(torch.zeros(2, 80, 10, device=DEV))
        m.model[0].conv.weight.mul_(1.0)
    with pytest.raises(ValueError, match='changed'):
        sess.push(torch.zeros(2, 80, 10, device=DEV))


def test_interleaved_whole_forwards_change_nothing():
    m = build(cases.ARCH_M, True, 'lively')
    x = keyed_input(2, 600, seed=4).to(DEV)
    y = keyed_input(3, 250, seed=6).to(DEV)
    with torch.no_grad():
        alone = m(y).clone()
        ref, _, _ = stream(m, x, [100] * 6)
        sess = m.stream(batch=2, max_chunk=160)
        outs = []
        for i in range(6):
            outs.append(sess.push(x[:, :, i * 100:(i + 1) * 100]))
            assert torch.equal(m(y), alone), i
        outs.append(sess.flush())
    assert torch.equal(torch.cat(outs, 1), ref)


def test_a_dropped_session_frees_its_memory_at_once():
    """No reference cycle through a session: the last reference gone, its buffers go back to the allocator without the cycle collector
    (which is off here) -- for the float32 and the bfloat16 session, after a push and a peek have made every lazily built part."""
    import gc
    import weakref
    gc.disable()
    try:
        for dtype in (torch.float32, torch.bfloat16):
            m = build(cases.ARCH_A, True, 'lively').to(dtype)
            sess = streaming.StreamingSession(m, 1, max_chunk=8, dtype=dtype)
            with torch.no_grad():
                sess.push(keyed_input(1, 8, seed=7).to(DEV).to(dtype))
                sess.peek()
            torch.cuda.synchronize()
            ref, owned, before = weakref.ref(sess), sess.buffer_bytes, torch.cuda.memory_allocated()
            del sess
            assert ref() is None, dtype
            assert before - torch.cuda.memory_allocated() >= owned > 0, dtype
    finally:
        gc.enable()
