"""A streaming session with both listeners, ``endpoint=`` and ``keywords=``: every push that emits frames ends with exactly one endpoint
step and then one keyword step, after the decode launches; both listeners hold what stand-alone streams fed the same logits hold; and
``peek_endpoint`` / ``peek_keywords`` between the pushes change neither the committed states nor anything a later push returns."""
import pytest
import torch

import cases
from nb_asr_amd import ctc, hip, streaming
from test_stream_launch_sequence_gpu import features, model_for

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SIZES = (40,) * 6 + (1,) + (40,) * 6             # feature frames per push; the first pushes are within the lookahead and emit no logit frame
LISTENERS = ['nbasr_ctc_endpoint_step', 'nbasr_ctc_keyword_step']


def same(a, b):
    if isinstance(a, torch.Tensor):
        return isinstance(b, torch.Tensor) and a.shape == b.shape and torch.equal(a, b)
    return len(a) == len(b) and all(same(u, v) for u, v in zip(a, b))


def run(decode, peeks):
    """One utterance through a session with both listeners -> (session, what each push and the flush returned, their tapes)."""
    sess = streaming.StreamingSession(model_for(cases.ARCH_M, True), 2, endpoint=ctc.EndpointRules(device=DEV),
                                      keywords=ctc.KeywordSet([(3, 4), (5,)], device=DEV))
    x = features(2, sum(SIZES), 3)
    outs, tapes, at = [], [], 0
    with torch.no_grad():
        for n in SIZES + (None,):
            entries = []
            hip.start_tape(entries)
            try:
                outs.append(sess.flush(decode=decode) if n is None else sess.push(x[..., at:at + n], decode=decode))
            finally:
                hip.stop_tape()
            tapes.append([e[0].__name__ for e in entries])
            if peeks and n is not None:
                committed = [sess._endpoint.state.clone(), sess._keywords.state.clone(), sess._endpoint._fresh, sess._keywords._fresh]
                ahead = sess.peek_endpoint(decode)[1], sess.peek_keywords(decode)[1]
                assert isinstance(ahead[0], ctc.EndpointResult) and isinstance(ahead[1], ctc.KeywordResult)
                assert same(committed[:2], [sess._endpoint.state, sess._keywords.state])
                assert committed[2:] == [sess._endpoint._fresh, sess._keywords._fresh]
            at += n or 0
    torch.cuda.synchronize()
    return sess, outs, tapes


@pytest.mark.parametrize('decode', [False, 'beam'])
def test_both_listeners_step_in_order_and_match_stand_alone_streams(decode):
    sess, outs, tapes = run(decode, peeks=False)
    ep, kw = ctc.EndpointStream(2, sess._endpoint.rules, DEV), ctc.KeywordStream(2, sess._keywords.keywords, DEV)
    emitted = []
    for out, names in zip(outs, tapes):
        logits = out if isinstance(out, torch.Tensor) else out[0]
        emitted.append(logits.shape[1])
        if logits.shape[1]:                      # the last two launches, and no other launch of either
            assert names[-2:] == LISTENERS and [names.count(name) for name in LISTENERS] == [1, 1]
            assert not decode or any('beam_stream' in name for name in names[:-2])
        else:
            assert not set(names) & set(LISTENERS)
        ep.push(logits)
        kw.push(logits)
    print('logit frames per push, then of the flush:', emitted)
    assert 0 in emitted[:-1] and sum(1 for m in emitted[:-1] if m) >= 3     # both kinds of push were seen
    assert torch.equal(sess.endpoint.state, ep.result.state) and torch.equal(sess.keywords.state, kw.result.state)
    assert int(sess.endpoint.frames[0]) == sum(emitted) and int(sess.keywords.frames[0, 0]) == sum(emitted)

    peeked, peeked_outs, _ = run(decode, peeks=True)
    assert same(peeked_outs, outs)
    assert torch.equal(peeked.endpoint.state, ep.result.state) and torch.equal(peeked.keywords.state, kw.result.state)
