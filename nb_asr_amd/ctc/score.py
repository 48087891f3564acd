"""Scoring and training: error rates, the CTC loss (value, and with its gradient for the training step), forced alignment, the evaluation loop."""
import collections

import torch

from . import _lengths, fold_table, hip, output_lengths
from .decode import beam_decode, log_softmax


def error_rates(hyp, hyp_len, ref, ref_len, blank=0, table=None):
    """Per-utterance token error rate, ``torch_edit_distance.compute_wer(hyp, ref, hyp_len, ref_len, blank, sep=[])``
    (trainer.py:245): Levenshtein distance / reference length, after mapping both sides through ``table`` (optional int32
    label table, e.g. ``fold_table()``) and dropping ``blank``.  Returns a float32 device tensor (B); an empty reference
    gives inf (nan when the hypothesis is empty too), as the division does in the reference."""
    dev = hyp.device
    b = hyp.shape[0]
    counts = hip.token_error_counts(hyp.to(torch.int32).contiguous(), _lengths(hyp_len, b, dev), ref.to(device=dev, dtype=torch.int32).contiguous(),
                                    _lengths(ref_len, b, dev), None if table is None else table.to(device=dev, dtype=torch.int32).contiguous(),
                                    blank)
    if bool((counts[:, 0] < 0).any()):
        raise hip.HipError('error_rates: a sequence exceeds 2048 tokens or holds a label outside the table')
    return counts[:, 0].float() / counts[:, 1].float()


def decode_per(log_probs, output_len, targets, targets_len, beam_width=12, fold_to=39, num_classes=48, *, lm=None, alpha=1.0, beta=0.0):
    """``Trainer.decode`` (trainer.py:229-247): best beam and targets folded to ``fold_to`` phonemes, error rate per
    utterance, mean over the batch.  ``log_probs`` (B, T', num_classes + 1) on the device; targets (B, L) labels of the
    ``num_classes`` set (0 = blank / padding).  Returns a 0-dim float32 device tensor.  ``lm``, ``alpha``, ``beta``: ``beam_decode``'s."""
    beams, _, beams_len = beam_decode(log_probs, output_len, beam_width=beam_width, lm=lm, alpha=alpha, beta=beta)
    table = fold_table(num_classes, fold_to).to(log_probs.device) if fold_to < num_classes else None
    per = error_rates(beams[:, 0].contiguous(), beams_len[:, 0].contiguous(), targets, targets_len, blank=0, table=table)
    return per.mean()


def ctc_loss(log_probs, output_len, targets, targets_len, blank=0):
    """The reference's loss value (``get_loss()``, trainer.py:36-42): ``F.ctc_loss(log_probs.permute(1, 0, 2), targets, output_len,
    targets_len, reduction='none', zero_infinity=True) / output_len`` averaged over the batch -- what ``Trainer.step`` reports
    for validation and test batches.  ``log_probs`` (B, T', C) stays batch-major on the device.  Forward value only (validation / test); the
    training step uses ``training_loss`` below."""
    dev = log_probs.device
    b = log_probs.shape[0]
    per = hip.ctc_loss(log_probs.contiguous(), _lengths(output_len, b, dev), targets.to(device=dev, dtype=torch.int32).contiguous(),
                       _lengths(targets_len, b, dev), blank, divide_by_length=True)
    return per.mean()


Alignment = collections.namedtuple('Alignment', ['path', 'score', 'starts', 'ends', 'token_scores'])


def forced_align(log_probs, output_len, targets, targets_len, blank=0):
    """CTC forced alignment (nbasr.h: nbasr_ctc_forced_align; torchaudio's ``forced_align`` + ``merge_tokens``): given the transcript, the
    best path through it and the frames of every token.  ``log_probs`` (B, T', C) float32 on the device, ``output_len`` and
    ``targets_len`` (B) tensors or sequences, ``targets`` (B, L) labels (never ``blank``).  Returns ``Alignment`` of device tensors:
    ``path`` (B, T') int32, the class at each frame (-1 beyond the utterance); ``score`` (B) float32, the path's log-probability;
    ``starts`` / ``ends`` (B, L) int32, first and one-past-last frame of each token (-1 beyond ``targets_len``; multiply by
    ``FRAME_SECONDS`` for seconds); ``token_scores`` (B, L) float32, each token's log-probability summed over its frames.  An utterance
    too short for its transcript has score -inf, path and spans -1; a label that is ``blank`` or outside the classes gives score NaN."""
    if not isinstance(log_probs, torch.Tensor) or log_probs.dim() != 3:
        raise ValueError(f'log_probs must be (batch, frames, classes), got {tuple(getattr(log_probs, "shape", ()))}')
    if log_probs.dtype != torch.float32 or not log_probs.is_cuda:
        raise ValueError(f'log_probs must be float32 on a HIP device (got {log_probs.dtype} on {log_probs.device}); this package has no CPU path')
    b, dev = log_probs.shape[0], log_probs.device
    if not isinstance(targets, torch.Tensor) or targets.dim() != 2 or targets.shape[0] != b:
        raise ValueError(f'targets must be ({b}, labels), got {tuple(getattr(targets, "shape", ()))}')
    scores, path, starts, ends, token_scores = hip.ctc_forced_align(
        log_probs.contiguous(), _lengths(output_len, b, dev), targets.to(device=dev, dtype=torch.int32).contiguous(), _lengths(targets_len, b, dev), int(blank))
    return Alignment(path, scores, starts, ends, token_scores)


def align(model, audio, audio_len, targets, targets_len):
    """``forced_align`` of a model's output: the ``eval()`` forward of ``audio`` (B, 80, T), ``log_softmax``, ``output_lengths(audio_len)``, then
    the alignment of ``targets`` -- which output frames (40 ms each, ``FRAME_SECONDS``) belong to which phoneme.  No gradients; the model's
    training flag is left as it was."""
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            log_probs = log_softmax(model(audio))
    finally:
        model.train(was_training)
    return forced_align(log_probs, output_lengths(torch.as_tensor(audio_len)), targets, targets_len)


def evaluation_step(model, audio, audio_len, targets, targets_len, beam_width=12):
    """``Trainer.step(inputs, training=False)`` followed by ``Trainer.decode`` (trainer.py:207-247) for one batch:
    forward -> log_softmax -> ``output_len = audio_len // 4`` -> loss value and phoneme error rate.
    ``audio`` (B, 80, T) on the model's device.  Returns ``(loss, per)`` as 0-dim device tensors."""
    with torch.no_grad():
        log_probs = log_softmax(model(audio))
    output_len = output_lengths(torch.as_tensor(audio_len))
    loss = ctc_loss(log_probs, output_len, targets, targets_len)
    per = decode_per(log_probs, output_len, targets, targets_len, beam_width=beam_width)
    return loss, per


def evaluate(model, batches, beam_width=12):
    """The reference's validation / test loop (trainer.py:150-158, 190-200): running averages of the per-batch loss and
    phoneme error rate (its ``AvgMeter``: every batch weighs the same).  ``batches`` yields
    ``((audio, audio_len), (targets, targets_len))`` like the reference's data loaders.  Returns ``(loss, per)`` floats."""
    was_training = model.training
    model.eval()
    n, loss_avg, per_avg = 0, 0.0, 0.0
    try:
        for (audio, audio_len), (targets, targets_len) in batches:
            loss, per = evaluation_step(model, audio, audio_len, targets, targets_len, beam_width)
            loss, per = loss.item(), per.item()
            if n == 0:
                loss_avg, per_avg = loss, per
            else:
                loss_avg = loss_avg * (n / (n + 1)) + loss / (n + 1)
                per_avg = per_avg * (n / (n + 1)) + per / (n + 1)
            n += 1
    finally:
        model.train(was_training)
    return loss_avg, per_avg


def ctc_loss_and_grad(log_probs, output_len, targets, targets_len, blank=0):
    """``ctc_loss`` together with the gradient of that scalar with respect to the LOGITS (``log_probs = log_softmax(logits)``):
    what the reference's ``loss.backward()`` hands to the model (trainer.py:220-223, without its weight-norm term).  Returns
    ``(loss, grad_logits)``; ``training_loss`` wraps it as an autograd function."""
    dev = log_probs.device
    b = log_probs.shape[0]
    per, grad = hip.ctc_loss_grad(log_probs.contiguous(), _lengths(output_len, b, dev), targets.to(device=dev, dtype=torch.int32).contiguous(),
                                  _lengths(targets_len, b, dev), blank)
    return per.mean(), grad


class _TrainingLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, output_len, targets, targets_len, blank):
        loss, grad = ctc_loss_and_grad(log_softmax(logits.detach().contiguous()), output_len, targets, targets_len, blank)
        ctx.save_for_backward(grad)
        return loss

    @staticmethod
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        return grad * g, None, None, None, None


def training_loss(logits, output_len, targets, targets_len, blank=0):
    """The trainer's loss on the LOGITS of a training-mode forward (trainer.py:215-223: ``log_softmax`` -> ``get_loss`` -> mean), attached
    to the autograd graph: ``training_loss(model.train()(x), ...).backward()`` reaches every parameter.  Loss and gradient with respect
    to the logits come from one HIP kernel pair (nbasr_ctc_loss_grad); add the reference's weight-norm term with torch if wanted."""
    return _TrainingLoss.apply(logits, output_len, targets, targets_len, blank)
