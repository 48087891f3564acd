"""The per-utterance chunk lengths of the three streams over the logits (``BeamSearchStream``, ``EndpointStream``, ``KeywordStream``) are
admitted by one helper, ``ctc._chunk_rows``, with the same three refusals.  None of the three can be made without a HIP device (each
allocates its state there), so the helper is tested directly."""
import pytest
import torch

from nb_asr_amd import ctc

ENDED = torch.tensor([False, True, False])


@pytest.mark.parametrize('lengths, message', [
    ([4, 0], r'expected 3 lengths, got 2'),
    (torch.zeros(2, 2), r'expected 3 lengths, got 4'),
    ([4, 0, 6], r'lengths must lie in \[0, 5\] for a chunk of 5 frames \(got \[4, 0, 6\]\)'),
    ([-1, 0, 5], r'lengths must lie in \[0, 5\] for a chunk of 5 frames \(got \[-1, 0, 5\]\)'),
    ([5, 1, 5], r'an utterance that has ended \(a chunk with fewer frames than the others\) cannot take more frames'),
    (None, r'an utterance that has ended \(a chunk with fewer frames than the others\) cannot take more frames'),
])
def test_length_refusals(lengths, message):
    with pytest.raises(ValueError, match=message):
        ctc._chunk_rows(lengths, 5, 3, ENDED)


@pytest.mark.parametrize('lengths', [[5, 0, 3], (0, 0, 0), torch.tensor([5, 0, 3], dtype=torch.int32), torch.tensor([[5.0], [0.0], [3.0]])])
def test_lengths_become_host_rows(lengths):
    rows = ctc._chunk_rows(lengths, 5, 3, ENDED)
    assert rows.dtype == torch.int64 and rows.device.type == 'cpu' and rows.tolist() == torch.as_tensor(lengths).reshape(-1).tolist()


def test_no_lengths_is_the_whole_chunk_for_every_utterance():
    assert ctc._chunk_rows(None, 5, 3, torch.zeros(3, dtype=torch.bool)).tolist() == [5, 5, 5]
    assert ctc._chunk_rows(None, 0, 3, ENDED).tolist() == [0, 0, 0]          # no frames: nothing for the ended utterance to refuse
