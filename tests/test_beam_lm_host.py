"""Bigram LM fusion of the beam search, the part that needs no GPU: the plain-Python model (beam_timesteps_model.py) with a zero table is
the model without one, its fused scores are log P_ctc + sum W by exhaustive enumeration, the seeds of the device
comparison hold no float32 tie, ``ctc.bigram_lm`` / ``ctc.fusion_table`` compute what they say, and the three new entry points are declared,
bound and refuse bad arguments on the host."""
import inspect

import numpy as np
import pytest
import torch

import beam_timesteps_model as model
from nb_asr_amd import ctc, hip, streaming
from nbasr_header import declarations
from oracle import decode_oracle as oracle

NAMES = ('nbasr_ctc_beam_search_lm', 'nbasr_ctc_beam_stream_lm_step', 'nbasr_ctc_beam_stream_lm_peek')
FLT_MAX = float(np.finfo(np.float32).max)


# ---- the model ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('shape', model.ORACLE_SHAPES)
def test_model_without_a_table_and_with_a_zero_table_is_the_unfused_model(shape):
    classes = shape[2]
    for key, lp, width, top_n in model.utterances(shape):
        want = model.beam_search(lp, width, cutoff_top_n=top_n)             # without a table: anchored on the oracle by test_beam_timesteps_host.py
        assert model.beam_search(lp, width, cutoff_top_n=top_n, fusion=np.zeros((classes, classes), np.float32)) == want, key


def test_fused_scores_are_the_exhaustive_ctc_scores_plus_the_bigram_sums():
    """A beam wide enough for every labelling, no pruning: the finite-score beams are exactly the labellings, ordered by and scored with
    log P_ctc(y) + sum_k W[y_{k-1}][y_k] (y_0 = blank).  1e-5 absolute: float32 round-off of fewer than 10 adds of O(10) values (1.4e-6
    was seen)."""
    worst, n_labellings = 0.0, 0
    for seed in range(40):
        frames, classes = ((4, 3), (3, 4))[seed % 2]
        rng = np.random.default_rng(seed)
        lp = torch.log_softmax(torch.from_numpy(1.5 * rng.normal(size=(frames, classes))), dim=1).to(torch.float32).numpy()
        W = rng.normal(size=(classes, classes)).astype(np.float32)
        got = [(tok, score) for tok, score, _ in model.beam_search(lp, 32, fusion=W) if score < 0.99 * FLT_MAX]
        want = []
        for lab, log_p in oracle.ctc_labelling_log_probs(lp).items():
            prev, total = 0, float(log_p)
            for c in lab:
                total += float(W[prev][c])
                prev = c
            want.append((list(lab), -total))
        want.sort(key=lambda e: e[1])
        assert [tok for tok, _ in got] == [tok for tok, _ in want], seed
        for (tok, score), (_, w_score) in zip(got, want):
            worst = max(worst, abs(score - w_score))
            assert abs(score - w_score) <= 1e-5, (seed, tok, score, w_score)
        n_labellings += len(want)
    print(f'{n_labellings} labellings, worst |score - exhaustive| {worst:.2e}')
    assert n_labellings >= 40 * 8


def test_fused_model_beams_do_not_hang_on_float32_ties():
    """A condition of the device comparison (test_beam_lm_gpu.py): at every utterance it uses, accumulating in float64 changes no beam."""
    changed = 0
    for shape in model.TIMED_SHAPES:
        W = model.fusion_table(shape[2])
        for key, lp, width, top_n in model.utterances(shape):
            f32 = model.beam_search(lp, width, cutoff_top_n=top_n, fusion=W)
            assert model.same_beams(f32, model.beam_search(lp, width, cutoff_top_n=top_n, fusion=W, dtype=np.float64)), key
            changed += not model.same_beams(f32, model.beam_search(lp, width, cutoff_top_n=top_n))
    assert changed >= 10                                           # the table matters: a search that ignored it could not pass


# ---- ctc.bigram_lm, ctc.fusion_table ------------------------------------------------------------------------------------------------

TRANSCRIPTS = torch.tensor([[1, 2, 1], [2, 2, 3], [1, 3, 3]])     # lengths 3, 2, 1: the 3s lie beyond them
LENGTHS = [3, 2, 1]


def test_bigram_lm_on_a_hand_counted_transcript_set():
    lm = ctc.bigram_lm(TRANSCRIPTS, LENGTHS, classes=4, blank=0, smoothing=1.0)
    assert lm.shape == (4, 4) and lm.dtype == torch.float32
    # first tokens 1, 2, 1; bigrams (1,2), (2,1), (2,2); class 3 is never seen
    counts = {0: [2, 1, 0], 1: [0, 1, 0], 2: [1, 1, 0], 3: [0, 0, 0]}
    for prev, row in counts.items():
        want = np.log((np.array(row) + 1.0) / (sum(row) + 3.0))
        np.testing.assert_allclose(lm[prev, 1:].numpy(), want, rtol=0, atol=1e-6)
        assert abs(float(torch.exp(lm[prev, 1:].double()).sum()) - 1.0) < 1e-6            # a distribution over the non-blank classes
        assert float(lm[prev, 0]) == float(lm[prev, 1:].min())                          # the blank column: the row's minimum
    assert torch.isfinite(lm).all()


def test_bigram_lm_honours_smoothing_and_blank():
    lm = ctc.bigram_lm(TRANSCRIPTS, LENGTHS, classes=4, blank=0, smoothing=0.25)
    np.testing.assert_allclose(lm[0, 1:].numpy(), np.log((np.array([2, 1, 0]) + 0.25) / 3.75), rtol=0, atol=1e-6)
    np.testing.assert_allclose(lm[2, 1:].numpy(), np.log((np.array([1, 1, 0]) + 0.25) / 2.75), rtol=0, atol=1e-6)
    # blank = 3: labels 0..2, row 3 holds the first tokens (0, 1, 0 after the shift)
    lm3 = ctc.bigram_lm(TRANSCRIPTS - 1, torch.tensor(LENGTHS), classes=4, blank=3)
    np.testing.assert_allclose(lm3[3, :3].numpy(), np.log((np.array([2, 1, 0]) + 1.0) / 6.0), rtol=0, atol=1e-6)
    np.testing.assert_allclose(lm3[1, :3].numpy(), np.log((np.array([1, 1, 0]) + 1.0) / 5.0), rtol=0, atol=1e-6)
    assert float(lm3[1, 3]) == float(lm3[1, :3].min())
    with pytest.raises(ValueError, match='blank'):
        ctc.bigram_lm(torch.tensor([[1, 0]]), [2], classes=4)     # blank is not a label
    with pytest.raises(ValueError, match='lengths'):
        ctc.bigram_lm(TRANSCRIPTS, [3, 2], classes=4)


def test_fusion_table_is_alpha_lm_plus_beta_in_float32():
    lm = np.random.default_rng(3).normal(size=(5, 5))
    table = ctc.fusion_table(torch.from_numpy(lm), 0.3, 1.7, 'cpu')
    assert table.dtype == torch.float32 and table.is_contiguous() and table.shape == (5, 5)
    want = lm.astype(np.float32) * np.float32(0.3) + np.float32(1.7)
    assert want.dtype == np.float32 and np.array_equal(table.numpy(), want)
    plain = ctc.fusion_table(torch.from_numpy(lm.astype(np.float32)).t(), 1.0, 0.0, 'cpu')          # a view: made contiguous
    assert plain.is_contiguous() and np.array_equal(plain.numpy(), lm.astype(np.float32).T)


@pytest.mark.parametrize('bad', [torch.zeros(3, 4), torch.zeros(5), torch.zeros(2, 3, 3), torch.zeros(65, 65), torch.zeros(0, 0)])
def test_fusion_table_refuses_wrong_shapes(bad):
    with pytest.raises(ValueError, match='classes'):
        ctc.fusion_table(bad, 1.0, 0.0, 'cpu')


@pytest.mark.parametrize('value', [float('nan'), float('inf'), float('-inf')])
def test_fusion_table_refuses_entries_that_are_not_finite(value):
    lm = torch.zeros(4, 4)
    lm[2, 1] = value
    with pytest.raises(ValueError, match='finite'):
        ctc.fusion_table(lm, 1.0, 0.0, 'cpu')
    with pytest.raises(ValueError, match='finite'):
        ctc.fusion_table(torch.zeros(4, 4), 1.0, value, 'cpu')


def test_python_interface_takes_the_lm_last_and_by_keyword():
    for fn in (ctc.beam_decode, ctc.decode_per, ctc.BeamSearchStream.__init__, streaming.StreamingSession.__init__):
        params = list(inspect.signature(fn).parameters.values())
        assert [p.name for p in params[-3:]] == ['lm', 'alpha', 'beta'], fn
        assert all(p.kind is inspect.Parameter.KEYWORD_ONLY for p in params[-3:]), fn
        assert [p.default for p in params[-3:]] == [None, 1.0, 0.0], fn
    assert [p.name for p in list(inspect.signature(ctc.beam_decode).parameters.values())[:5]] == ['log_probs', 'output_len', 'beam_width', 'blank',
                                                                                                 'cutoff_top_n']


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', NAMES)
def test_symbols_are_declared_and_bound_with_the_header_signature(name):
    """That the binding's types are the header's is test_abi.py's check of every symbol."""
    ret, args = declarations()[name]
    restype, argtypes = hip.SIGNATURES[name]
    assert ret == 'int' and restype is hip.ctypes.c_int
    assert any('fusion' in a for a in args) and args[-2] == 'int timed'
    assert getattr(hip.load_library(), name).argtypes == argtypes
    assert hip.load_library().nbasr_version() == 6


def _refused(rc, lib, word):
    assert rc < 0 and word in lib.nbasr_last_error(), (rc, lib.nbasr_last_error())


def test_fused_entry_points_refuse_bad_arguments_on_the_host():
    lib = hip.load_library()
    p = 16                                            # a non-NULL, 8-byte aligned stand-in: every case is refused before a launch

    def search(fusion=p, classes=49, width=12, timed=0, timesteps=None, batch=1):
        #      log_probs, lengths, fusion, ws, beams, scores, timesteps, beam_lens, batch, frames, classes, width, blank, top_n, timed, stream
        return lib.nbasr_ctc_beam_search_lm(p, None, fusion, p, p, p, timesteps, p, batch, 10, classes, width, 0, 40, timed, None)

    def step(fusion=p, classes=49, width=12, timed=0, frames=None):
        #      log_probs, lengths, fusion, state, ws, committed, c_frames, c_counts, partial, p_frames, p_counts, usage, batch, frames, classes, ...
        return lib.nbasr_ctc_beam_stream_lm_step(p, None, fusion, p, p, p, frames, p, p, frames, p, p, 1, 10, classes, width, 0, 40, 1000, timed, None)

    def peek(fusion=p, classes=49, width=12, timed=0, timesteps=None):
        #      log_probs, lengths, fusion, state, ws, beams, scores, timesteps, beam_lens, ld, batch, frames, classes, width, blank, top_n, pool, timed
        return lib.nbasr_ctc_beam_stream_lm_peek(p, None, fusion, p, p, p, p, timesteps, p, 20, 1, 10, classes, width, 0, 40, 1000, timed, None)

    for call in (search, step, peek):
        _refused(call(fusion=None), lib, b'fusion')
        _refused(call(classes=65), lib, b'unsupported')
        _refused(call(width=33), lib, b'unsupported')
        _refused(call(timed=1), lib, b'NULL')          # the timed outputs are missing
    _refused(search(fusion=None, batch=0), lib, b'fusion')         # the table is part of the call even when there is nothing to do
