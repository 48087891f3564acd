"""The step after the forward pass: log_softmax, length mapping, CTC decoding, phoneme error rate.

Mirrors what the reference's ``Trainer.step`` / ``Trainer.decode`` do with the model output
(``training/torch/trainer.py:217-219, 229-247``): ``output = F.log_softmax(output, dim=2)``,
``output_len = audio_len // 4``, then ``CTCBeamDecoder(vocab, beam_width=12, log_probs_input=True).decode`` (ctcdecode,
third-party C++, not in the reference's tree), ``PhonemeEncoder.fold_encoded(., 39)`` on the best beam and on the targets,
``torch_edit_distance.compute_wer`` and the mean.  All of it runs on the device: ``beam_decode`` (prefix beam search),
``fold_table`` (the 48 -> 39 label table, with the reference's relabelling order), ``error_rates`` (label table + blank
removal + Levenshtein distance) and ``decode_per`` = the whole of ``Trainer.decode``.  ``greedy_decode`` is the cheap
width-1 relative (per-frame argmax, collapse, drop blank).  Beside the decoders, with no reference counterpart: ``forced_align``
(which frames belong to which phoneme), ``endpoint`` / ``EndpointStream`` (when has the utterance ended), ``spot_keywords`` /
``KeywordStream`` (has this phrase just been said), ``segment`` / ``SegmentStream`` (where are the stretches of speech in a stream
that goes on), with ``decode_spans`` to transcribe them, and ``confidence`` / ``path_confidence`` / ``ConfidenceStream`` (how sure is the
recogniser of each token).
"""
import inspect

import torch

from .. import hip  # noqa: F401  (part of this module's interface)
from ..frontend import LogMelFrontend
from ..phonemes import fold_table  # noqa: F401  (part of this module's interface)

OUTPUT_STRIDE = 4                 # input frames per output frame: the model's two stride-2 convolutions
_FRONTEND = inspect.signature(LogMelFrontend.__init__).parameters
# seconds per output frame: the front-end's hop (160 samples at 16 kHz = 10 ms) times the model's stride = 40 ms; turns frame spans into seconds
FRAME_SECONDS = OUTPUT_STRIDE * _FRONTEND['hop_length'].default / _FRONTEND['sample_rate'].default


def output_lengths(audio_len):
    """Frames of the model output that belong to each utterance: ``audio_len // 4`` (trainer.py:219).  Note this is the
    trainer's convention, not ceil(ceil(T/2)/2): for T not divisible by 4 the last partial output frame is ignored."""
    return torch.div(audio_len, OUTPUT_STRIDE, rounding_mode='floor')


def _lengths(lengths, batch, device):
    if lengths is None:
        return None
    lengths = torch.as_tensor(lengths)
    if lengths.numel() != batch:
        raise ValueError(f'expected {batch} lengths, got {lengths.numel()}')
    return lengths.to(device=device, dtype=torch.int32).contiguous()


def _positive(batch):
    batch = int(batch)
    if batch < 1:
        raise ValueError(f'batch must be positive (got {batch})')
    return batch


def _chunk_rows(lengths, n, batch, ended):
    """Each utterance's frames in a chunk of ``n`` frames, as every stream over the logits admits them: int64 (B) on the host from
    ``lengths`` (None: all ``n``; a device tensor is read back).  ``ended``: bool (B), the utterances an earlier chunk gave fewer frames."""
    if lengths is None:
        rows = torch.full((batch,), n, dtype=torch.int64)
    else:
        rows = torch.as_tensor(lengths).reshape(-1).to(torch.int64).cpu()
        if rows.numel() != batch:
            raise ValueError(f'expected {batch} lengths, got {rows.numel()}')
        if bool(((rows < 0) | (rows > n)).any()):
            raise ValueError(f'lengths must lie in [0, {n}] for a chunk of {n} frames (got {rows.tolist()})')
    if bool((ended & (rows > 0)).any()):
        raise ValueError('an utterance that has ended (a chunk with fewer frames than the others) cannot take more frames')
    return rows


# the families: each defines its names from the ones bound above (``*`` skips their private names)
from .decode import *       # noqa: E402,F401,F403
from .decode import _fusion, _cut_rows      # noqa: E402,F401
from .detect import *       # noqa: E402,F401,F403
from .detect import _DeviceTables, _RecordView, _logit_chunk, _LogitDetectorStream, _SpeechDecision, _spec, _whole, _class_count      # noqa: E402,F401
from .record_detectors import *   # noqa: E402,F401,F403
from .record_detectors import _NEG_INF_BITS, _fresh_endpoint_state, _fresh_segment_state, _fresh_keyword_state, _segment_rules      # noqa: E402,F401
from .score import *        # noqa: E402,F401,F403
from .score import _TrainingLoss      # noqa: E402,F401
from .token_confidence import *   # noqa: E402,F401,F403
from .token_confidence import _sum64, _mean_of, _fresh_confidence_state, _confidence_rules, _confidence_step      # noqa: E402,F401
