"""Confidence: how sure is the recogniser of each token? (nbasr.h "confidence"; DESIGN.md §9 "Confidence")"""
import torch

from . import _lengths, _positive, hip
from .detect import _class_count, _DeviceTables, _LogitDetectorStream, _spec, _whole, _whole_utterances
from .score import forced_align

CONFIDENCE_MEASURES = hip.CONFIDENCE_MEASURES
CONFIDENCE_ONE = 1 << 24         # the quantised confidence of 1.0: q = rint(conf * 2^24)


class ConfidenceRules(_DeviceTables):
    """What the confidence estimator measures with: ``measure``, how a frame's softmax becomes a number in [0, 1] -- ``'prob'``, the
    probability of the frame's label; ``'entropy'``, one minus the Gibbs entropy over ``ln(classes)``; ``'tsallis'``, the Tsallis entropy
    of order ``alpha`` normalised the same way (Laptev and Ginsburg 2022) -- ``alpha`` (read by ``'tsallis'``), the ``blank``
    class and ``classes``.  A token's confidence is the mean and the minimum of its frames' numbers.

    The defaults are the paper's choice for CTC models, Tsallis at alpha = 1/3.  They are UNTUNED for this model: starting points, not
    recommendations; no threshold on the result is offered here.

    Validates as the C side does (``ValueError``): a known measure, ``alpha`` a number strictly between 0 and 1, 2..128 classes, ``blank``
    one of them.  Everything travels by value: there is no device table (``device`` only names where a stream made from these rules
    lives by default)."""

    OWNER, THINGS, SHOWN = 'the confidence estimator', 'the confidence rules', ('measure', 'alpha', 'blank', 'classes')

    def __init__(self, measure='tsallis', alpha=1 / 3, blank=0, classes=49, device=None):
        if measure not in CONFIDENCE_MEASURES:
            raise ValueError(f'measure must be one of {CONFIDENCE_MEASURES} (got {measure!r})')
        if isinstance(alpha, bool) or not isinstance(alpha, (int, float)) or not 0.0 < float(alpha) < 1.0:
            raise ValueError(f'alpha must be a number strictly between 0 and 1 (got {alpha!r})')
        for name, v in (('classes', classes), ('blank', blank)):
            if not _whole(v):
                raise ValueError(f'{name} must be an integer (got {v!r})')
        classes, blank = _class_count(classes, blank)
        self.measure, self.alpha, self.blank, self.classes = measure, float(alpha), blank, classes
        self.measure_index = CONFIDENCE_MEASURES.index(measure)
        self._set_device(device)


def _sum64(lo, hi):
    """(lo, hi) int32 bit patterns -> the int64 they spell."""
    return (hi.to(torch.int64) << 32) | (lo.to(torch.int64) & 0xFFFFFFFF)


def _mean_of(sum_q, frames):
    """float32(double(sum_q) / (double(frames) * 2^24)), NaN where there is no frame: the one way a mean is made from the integers."""
    frames = frames.to(torch.float64)
    mean = sum_q.to(torch.float64) / (frames * float(CONFIDENCE_ONE))
    return torch.where(frames > 0, mean, float('nan')).to(torch.float32)


class ConfidenceResult:
    """The tokens one step closed, and the utterance so far.  Device tensors, all made from the integers the kernel wrote (a state record
    (B, 16) and the step's token table (B, n + 1, 8) with its counts): ``counts`` (B) int32, the tokens this step closed; ``labels``,
    ``starts``, ``ends``, ``min_q`` (B, n + 1) int32 and ``sum_q`` (B, n + 1) int64, token k of a row in column k, -1 past the row's count;
    a token is the frames ``[start, end)`` since the stream's start, ``min_q`` and ``sum_q`` the minimum and the sum of its frames'
    quantised confidences ``rint(conf * 2^24)``; ``mean`` and ``min`` (B, n + 1) float32 in [0, 1], NaN past the count: ``float32(double(
    sum_q) / (double(end - start) * 2^24))`` and ``float32(min_q) * 2^-24``.  Of the utterance, (B): ``frames`` (frames seen), ``tokens``
    (tokens closed so far, in all), ``bad`` (1 once a path label fell outside the classes), ``utterance_mean`` and ``utterance_min``
    (float32, over every frame of a token so far -- an open token's included; NaN and 1.0 before the first).  Only ``tokens_list()``
    reads the device.  The utterance's tensors are columns of the state record: a stream's result moves with its next step (a peek's
    with the next peek); the token table is the step's own."""

    def __init__(self, state, table, counts):
        self.state, self.table, self.counts = state, table, counts       # (B, 16), (B, n + 1, 8), (B) int32: a step makes one of these, so
                                                                         # the views below are made when asked for
    labels = property(lambda self: self.table[:, :, 0])
    starts = property(lambda self: self.table[:, :, 1])
    ends = property(lambda self: self.table[:, :, 2])
    min_q = property(lambda self: self.table[:, :, 3])
    frames = property(lambda self: self.state[:, 0])
    tokens = property(lambda self: self.state[:, 6])
    bad = property(lambda self: self.state[:, 11])

    @property
    def sum_q(self):
        return torch.where(self.labels >= 0, _sum64(self.table[:, :, 4], self.table[:, :, 5]), -1)

    @property
    def mean(self):
        return _mean_of(self.sum_q, torch.where(self.labels >= 0, self.ends - self.starts, 0))

    @property
    def min(self):
        return torch.where(self.labels >= 0, self.min_q.to(torch.float32) * (1.0 / CONFIDENCE_ONE), float('nan'))

    @property
    def utterance_mean(self):
        return _mean_of(_sum64(self.state[:, 8], self.state[:, 9]), self.state[:, 10])

    @property
    def utterance_min(self):
        return self.state[:, 7].to(torch.float32) * (1.0 / CONFIDENCE_ONE)

    def tokens_list(self):
        """The tokens as host values -- the one method here that reads the device.  Per row a list of ``(label, start, end, mean, min)``
        in the order they closed, ``mean`` and ``min`` python floats holding the float32 values."""
        counts, table = self.counts.cpu().tolist(), self.table.cpu()
        mean, least = self.mean.cpu().tolist(), self.min.cpu().tolist()
        return [[(*table[b, k, :3].tolist(), mean[b][k], least[b][k]) for k in range(counts[b])] for b in range(len(counts))]

    def __repr__(self):
        return f'ConfidenceResult(frames={self.frames.tolist()}, tokens={self.tokens.tolist()}, counts={self.counts.tolist()})'


def _fresh_confidence_state(batch):
    """(B, 16) int32 on the host: the fresh rows of nbasr.h."""
    return torch.tensor([[0, -1, -1, CONFIDENCE_ONE, 0, 0, 0, CONFIDENCE_ONE] + [0] * 8] * batch, dtype=torch.int32).reshape(batch, hip.CONFIDENCE_STATE_WORDS)


def _confidence_rules(rules, device=None):
    return _spec(rules, ConfidenceRules, 'rules', device)


def _confidence_step(rules, x, lengths, path, state_in, state_out, final, frame_q=None):
    """One launch of nbasr_ctc_confidence_step with a token table of its own -> the ``ConfidenceResult`` of ``state_out`` and that table."""
    b, n, _ = x.shape
    table = torch.empty(b, n + 1, hip.CONFIDENCE_TOKEN_WORDS, dtype=torch.int32, device=x.device)
    counts = torch.empty(b, dtype=torch.int32, device=x.device)
    hip.ctc_confidence_step(x, lengths, path, state_in, state_out, rules.measure_index, rules.alpha, rules.blank, final, table, counts, frame_q)
    return ConfidenceResult(state_out, table, counts)


def confidence(x, output_len=None, rules=None, path=None, return_frames=False):
    """How sure is the recogniser of each token of these utterances?  ``x`` (B, T', C) float32 logits or log-probabilities on the device
    (the result is the same for both), ``output_len`` their valid frames (tensor, sequence or None), ``rules`` a ``ConfidenceRules``
    (None: the defaults, 49 classes).  The tokens are ``greedy_decode``'s: maximal runs of one non-blank argmax.  ``path`` (B, T') int32
    gives the labels of another hypothesis frame by frame instead -- ``forced_align``'s ``path`` for a beam result (``path_confidence``
    does both); a label outside the classes counts as blank and sets ``bad``.  Returns a ``ConfidenceResult`` of every token -- with
    ``return_frames=True`` ``(result, frames)``, frames (B, T') float32: each frame's confidence, blanks included, NaN beyond an
    utterance's length.  A fresh state and one final step of the kernel the streams run (nbasr_ctc_confidence_step): the same bits
    as any chunking of the frames."""
    rules = _confidence_rules(rules)
    x, (b, n, _), lengths, state = _whole_utterances(x, output_len, rules, hip.CONFIDENCE_STATE_WORDS)
    if path is not None:
        if not isinstance(path, torch.Tensor) or tuple(path.shape) != (b, n):
            raise ValueError(f'path must be a ({b}, {n}) tensor of labels, got {tuple(getattr(path, "shape", ()))}')
        path = path.to(device=x.device, dtype=torch.int32).contiguous()
    frame_q = torch.empty(b, n, dtype=torch.int32, device=x.device) if return_frames else None
    if b:
        result = _confidence_step(rules, x, lengths, path, None, state, True, frame_q)
    else:
        result = ConfidenceResult(state, torch.empty(0, n + 1, hip.CONFIDENCE_TOKEN_WORDS, dtype=torch.int32, device=x.device), state[:, 0])
    if not return_frames:
        return result
    return result, torch.where(frame_q >= 0, frame_q.to(torch.float32) * (1.0 / CONFIDENCE_ONE), float('nan'))


def path_confidence(log_probs, output_len, targets, targets_len, rules=None):
    """The confidence of a given transcript: ``forced_align(log_probs, output_len, targets, targets_len)``, then ``confidence`` along its
    ``path``.  The tokens of the ``ConfidenceResult`` are the targets, ``starts`` and ``ends`` their aligned frames -- how a hypothesis
    other than the greedy one (a beam result) gets confidences.  A row without a path (the aligner's score is -inf or NaN: too short
    for its transcript, a label that is blank or no class) gets no tokens and no frames.  Two launches, no synchronisation."""
    rules = _confidence_rules(rules)
    found = forced_align(log_probs, output_len, targets, targets_len, rules.blank)
    b, n, _ = log_probs.shape
    lengths = _lengths(output_len, b, log_probs.device)
    if lengths is None:
        lengths = torch.full((b,), n, dtype=torch.int32, device=log_probs.device)
    lengths = torch.where(torch.isfinite(found.score), lengths, 0).to(torch.int32)
    return confidence(log_probs, lengths, rules, path=found.path)


class ConfidenceStream(_LogitDetectorStream):
    """``confidence`` fed chunk by chunk (nbasr_ctc_confidence_step with a carried state; DESIGN.md §9 "Confidence").

        cf = ConfidenceStream(batch, rules, device=dev)
        r = cf.push(logits_chunk, lengths=None)  # ConfidenceResult of the tokens this push closed; all pushes together == confidence(all frames)
        r = cf.finish()                          # a final step of no frames: closes the token that is still open
        r = cf.peek(next_chunk)                  # what push(next_chunk, final=True) would close; the stream stays as it was
        cf.last                                  # the latest step's result; cf.reset() starts the next utterances

    A ``_LogitDetectorStream`` -- the three records, ``lengths``, ``reset()`` and the refusals are the base's -- whose steps differ in two
    ways: a result holds the tokens its own step closed (a token closes at the first frame that does not continue it, so the last one
    stays open until a final step), and a step can be final.  ``push(x, final=True)`` or ``finish()`` ends the rows: they take no more
    frames until ``reset()``.  A push of no frames that is not final launches nothing, and neither does ``reset()``.  ``peek`` is final
    by default -- it answers "if the audio stopped here" -- and ``peek()`` without frames shows what ``finish()`` would close.
    ``state_bytes`` counts the base's records and the constant empty token table a step without a launch answers with."""

    RESULT = ConfidenceResult

    def __init__(self, batch, rules=None, device=None):
        batch, self.rules = _positive(batch), _confidence_rules(rules, device)
        self._nothing = None                     # the constant table and counts of a step that closed nothing, made with the first result
        super().__init__(batch, self.rules, device)

    def _fresh_rows(self):
        return _fresh_confidence_state(self.batch)

    @property
    def state_bytes(self):
        return super().state_bytes + sum(t.numel() * t.element_size() for t in self._nothing)

    def reset(self):
        """Start a new batch of utterances.  No launch: the next step starts from fresh rows."""
        super().reset()
        self.final = False
        self.last = self.result

    @property
    def result(self):
        """The committed record with no tokens: what a step that launched nothing answers with."""
        if self._nothing is None:
            self._nothing = (torch.full((self.batch, 1, hip.CONFIDENCE_TOKEN_WORDS), -1, dtype=torch.int32).to(self.device),
                             torch.zeros(self.batch, dtype=torch.int32).to(self.device))
        return ConfidenceResult(self._fresh_state if self._fresh else self.state, *self._nothing)

    def _chunk(self, x, lengths):
        if x is None:
            x = torch.empty(self.batch, 0, self._classes, dtype=torch.float32, device=self.device)
        x, n, rows, chunk_lengths = super()._chunk(x, lengths)
        if self.final and n:
            raise ValueError('the utterances have ended (a final step): call reset() to start the next ones')
        return x, n, rows, chunk_lengths

    def push(self, x, lengths=None, final=False):
        """Take the next chunk (B, n, C) of logits or log-probabilities; returns the ``ConfidenceResult`` of the tokens this push closed.
        ``final``: the rows end with this chunk, which closes the token that is open."""
        x, n, rows, chunk_lengths = self._chunk(x, lengths)
        if self.final and final:
            raise ValueError('the utterances have ended (a final step): call reset() to start the next ones')
        if n or final:
            self.last = _confidence_step(self.rules, x, chunk_lengths, None, None if self._fresh else self.state, self.state, final)
            self._fresh = False
            if rows is not None:
                self.ended |= rows < n
            self.final = bool(final)
        else:
            self.last = self.result
        return self.last

    def finish(self):
        """End the utterances: a final step of no frames (one launch)."""
        return self.push(None, final=True)

    def peek(self, x=None, lengths=None, final=True):
        """The result ``push(x, lengths, final)`` would return, with the stream left as it was (the committed record is only read).
        ``x`` None: no frames.  No frames and not final, or after a final step: ``result``, no launch."""
        x, n, _, chunk_lengths = self._chunk(x, lengths)
        if not n and (self.final or not final):
            return self.result
        if self._peek_state is None:
            self._peek_state = torch.empty_like(self.state)
        return _confidence_step(self.rules, x, chunk_lengths, None, None if self._fresh else self.state, self._peek_state, final)
