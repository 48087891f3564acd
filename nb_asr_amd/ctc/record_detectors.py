"""The detectors whose result is a view of one state record: endpoint, segments, keywords (nbasr.h and DESIGN.md §9 "Endpoint", "Segments", "Keywords")."""
import torch

from . import FRAME_SECONDS, _positive, hip
from .detect import _class_count, _DeviceTables, _LogitDetectorStream, _RecordView, _spec, _SpeechDecision, _whole, _whole_utterances

MAX_ENDPOINT_RULES = 8
MAX_SEGMENT_CAPACITY = hip.SEGMENT_MAX_CAPACITY
MAX_KEYWORDS = 64
MAX_KEYWORD_TOKENS = hip.KEYWORD_MAX_TOKENS
_NEG_INF_BITS = -8388608         # float32 -inf as an int32


class EndpointRules(_SpeechDecision):
    """What the endpointer decides with: the speech classes, the margin, and up to 8 rules ``(min_speech, min_trailing, min_frames)`` in
    output frames (40 ms each, ``FRAME_SECONDS``).  A frame is speech iff its largest value over ``speech_classes`` exceeds its largest
    value over the other classes by more than ``margin`` (logits and log-probabilities give the same answer); a rule holds at a frame
    when the utterance has at least ``min_speech`` speech frames, ``min_trailing`` frames since the last one (all frames, while there
    is none) and ``min_frames`` frames in all; the first frame at which a rule holds is the endpoint, the lowest such rule its rule.

    The defaults read: 5 s of silence with nothing said; 1 s of silence after speech; 20 s in all -- Kaldi's online-endpoint rules 1, 3
    and 5 in 40 ms frames.  They are UNTUNED for this model: starting points, not recommendations.

    Validates as the C side does (``ValueError``): 2..128 classes, a speech set that is neither empty nor every class and names no
    class outside them, 1..8 rules of three non-negative int32 values, a margin that is a number >= 0.  Owns the device table of the
    rules, made once, by the first step that needs it (``device`` None: the current HIP device)."""

    OWNER, THINGS, SHOWN = 'the endpointer', 'the rules', ('rules', 'speech_classes', 'margin', 'classes')

    def __init__(self, rules=((0, 125, 0), (1, 25, 0), (0, 0, 500)), speech_classes=None, margin=0.0, classes=49, device=None):
        self._set_speech(speech_classes, margin, classes)
        rules = tuple(tuple(rule) for rule in rules)
        if not 1 <= len(rules) <= MAX_ENDPOINT_RULES:
            raise ValueError(f'there must be 1 to {MAX_ENDPOINT_RULES} rules (got {len(rules)})')
        for rule in rules:
            if len(rule) != 3 or not all(_whole(v, 2 ** 31) for v in rule):
                raise ValueError(f'a rule is (min_speech, min_trailing, min_frames), non-negative int32 frame counts (got {rule})')
        self.rules = tuple(tuple(int(v) for v in rule) for rule in rules)
        self._set_device(device)

    @staticmethod
    def frames_for(seconds):
        """Seconds -> frames: the seconds to the millisecond, then the smallest frame count that covers them (1.0 -> 25, 0.05 -> 2)."""
        ms, frame_ms = round(float(seconds) * 1000), round(FRAME_SECONDS * 1000)
        if ms < 0:
            raise ValueError(f'a duration must not be negative (got {seconds} s)')
        return -(-ms // frame_ms)

    @classmethod
    def from_seconds(cls, rules=((0.0, 5.0, 0.0), (0.04, 1.0, 0.0), (0.0, 0.0, 20.0)), **kwargs):
        """The rules given as ``(min_speech, min_trailing, min_total)`` in seconds (``frames_for`` converts each); the other arguments
        are the constructor's.  The defaults are the constructor's."""
        return cls(tuple(tuple(cls.frames_for(v) for v in rule) for rule in rules), **kwargs)

    def _build(self, device):
        return torch.tensor(self.rules, dtype=torch.int32).to(device).contiguous()

    def table_on(self, device):
        """The rules as an (n_rules, 3) int32 tensor on ``device``, made by the first call; a rule set lives on one device."""
        return self._on(device)

    @property
    def table(self):
        """The device table (``device`` None or without an index: on the current HIP device)."""
        return self._here()


class EndpointResult(_RecordView):
    """The endpointer's view of a batch: int32 device tensors (B) ``frames`` (frames seen), ``speech_frames``, ``first_speech`` and
    ``last_speech`` (frame indices, -1: none yet), ``endpoint_frame`` (the frame at which the first rule held, -1: no endpoint yet)
    and ``rule`` (that rule's index, -1).  Nothing here reads the device: ``bool((r.endpoint_frame >= 0).any())`` is the caller's
    synchronisation.  The tensors are columns of the state record they were made from: a stream's ``result`` shows its committed
    record and moves with the next ``push`` or ``reset()``, a peek's shows the peek record until the next ``peek``; ``clone()`` keeps one."""

    FIELDS = ('frames', 'speech_frames', 'first_speech', 'last_speech', 'endpoint_frame', 'rule')
    WORDS = {name: (k, torch.int32) for k, name in enumerate(FIELDS)}       # of a record (B, 8) int32

    def seconds(self):
        """(``endpoint_frame``, ``first_speech``, ``last_speech``) as float32 device tensors of seconds from the utterance's start:
        the START of each frame, ``frame * FRAME_SECONDS``; -1 frames stay -1.0."""
        return tuple(self._frame_seconds(t) for t in (self.endpoint_frame, self.first_speech, self.last_speech))


def _fresh_endpoint_state(batch):
    """(B, 8) int32 on the host: the fresh rows of nbasr.h."""
    return torch.tensor([[0, 0, -1, -1, -1, -1, 0, 0]] * batch, dtype=torch.int32)


def endpoint(x, output_len=None, rules=None, return_mask=False):
    """Where do these utterances end?  ``x`` (B, T', C) float32 logits or log-probabilities on the device, ``output_len`` their valid
    frames (tensor, sequence or None), ``rules`` an ``EndpointRules`` (None: the defaults, 49 classes).  Returns an ``EndpointResult``
    -- with ``return_mask=True`` ``(result, mask)``, mask (B, T') uint8: 1 where the frame is speech, 0 beyond an utterance's length.
    A fresh state and one step of the kernel the streams run (nbasr_ctc_endpoint_step): the same bits as any chunking of the frames."""
    rules = _spec(rules, EndpointRules, 'rules')
    x, (b, n, _), lengths, state = _whole_utterances(x, output_len, rules, hip.ENDPOINT_STATE_WORDS)
    mask = torch.empty(b, n, dtype=torch.uint8, device=x.device) if return_mask else None
    if b:
        hip.ctc_endpoint_step(x, lengths, None, state, rules.table_on(x.device), rules.speech_lo, rules.speech_hi, rules.margin, mask)
    return (EndpointResult(state), mask) if return_mask else EndpointResult(state)


class EndpointStream(_LogitDetectorStream):
    """``endpoint`` fed chunk by chunk (nbasr_ctc_endpoint_step with a carried state; DESIGN.md §9 "Endpoint").

        ep = EndpointStream(batch, rules, device=dev)
        r = ep.push(logits_chunk, lengths=None)  # EndpointResult of everything pushed: == endpoint(all frames), bit for bit
        r = ep.peek(next_chunk)                  # what push(next_chunk) would return; the stream stays as it was
        ep.result                                # the committed result; ep.reset() starts the next utterances

    The push / peek / reset contract is ``_LogitDetectorStream``'s.  ``lengths`` (B) gives each utterance's frames in this chunk, as in
    ``BeamSearchStream.push``: fewer than the chunk has ends that utterance, and it takes no frames after that (host values cost no
    synchronisation; a device tensor is read back).  A push of no frames launches nothing, and neither does ``reset()``."""

    RESULT = EndpointResult

    def __init__(self, batch, rules=None, device=None):
        batch, self.rules = _positive(batch), _spec(rules, EndpointRules, 'rules', device)
        super().__init__(batch, self.rules, device)

    def _fresh_rows(self):
        return _fresh_endpoint_state(self.batch)

    def _step(self, x, chunk_lengths, state_out):
        r = self.rules
        hip.ctc_endpoint_step(x, chunk_lengths, None if self._fresh else self.state, state_out, self._tables, r.speech_lo, r.speech_hi, r.margin)


class SegmentRules(_SpeechDecision):
    """What the segmenter decides with: the endpointer's speech decision (``speech_classes``, ``margin``, ``classes``) and three counts
    in output frames (40 ms each, ``FRAME_SECONDS``).  ``min_speech`` consecutive speech frames open a segment, at the first of them;
    ``min_silence`` consecutive other frames close it, at the first of them (reason 0), so shorter pauses stay inside a segment;
    a segment that reaches ``max_frames`` frames is closed there by force (reason 1) and the next one needs ``min_speech`` new speech
    frames (0: no limit).  Unlike the endpoint, nothing latches: segments open and close for as long as frames arrive, and each row
    keeps its last ``capacity`` closed segments in a ring on the device.

    The defaults read: 120 ms of speech open a segment, half a second of silence closes it, no forced close, the last 16 segments.
    They are UNTUNED for this model: starting points, not recommendations.

    Validates as the C side does (``ValueError``): the speech decision as ``EndpointRules`` does; ``min_speech`` and ``min_silence``
    int32 values >= 1; ``max_frames`` 0 or an int32 value above ``min_speech``; ``capacity`` in [1, 64].  The counts travel by value:
    there is no device table (``device`` only names where a stream made from these rules lives by default)."""

    OWNER, THINGS = 'the segmenter', 'the segment rules'
    SHOWN = ('min_speech', 'min_silence', 'max_frames', 'capacity', 'speech_classes', 'margin', 'classes')

    def __init__(self, min_speech=3, min_silence=13, max_frames=0, capacity=16, speech_classes=None, margin=0.0, classes=49, device=None):
        self._set_speech(speech_classes, margin, classes)
        for name, v in (('min_speech', min_speech), ('min_silence', min_silence), ('max_frames', max_frames), ('capacity', capacity)):
            if not _whole(v, 2 ** 31):
                raise ValueError(f'{name} must be a non-negative int32 count (got {v})')
        min_speech, min_silence, max_frames, capacity = int(min_speech), int(min_silence), int(max_frames), int(capacity)
        if min_speech < 1 or min_silence < 1:
            raise ValueError(f'min_speech and min_silence must be at least 1 frame (got {min_speech}, {min_silence})')
        if max_frames and max_frames <= min_speech:
            raise ValueError(f'max_frames must be 0 (no limit) or above min_speech={min_speech} (got {max_frames})')
        if not 1 <= capacity <= MAX_SEGMENT_CAPACITY:
            raise ValueError(f'capacity must lie in [1, {MAX_SEGMENT_CAPACITY}] (got {capacity})')
        self.min_speech, self.min_silence, self.max_frames, self.capacity = min_speech, min_silence, max_frames, capacity
        self._set_device(device)

    @classmethod
    def from_seconds(cls, min_speech=0.12, min_silence=0.5, max_seconds=0.0, **kwargs):
        """The three counts given in seconds (``EndpointRules.frames_for`` converts each: the smallest frame count that covers them);
        the other arguments are the constructor's.  The defaults are the constructor's."""
        return cls(*(EndpointRules.frames_for(v) for v in (min_speech, min_silence, max_seconds)), **kwargs)

    @property
    def counts(self):
        """``(min_speech, min_silence, max_frames, capacity)``: what a step is handed by value, in its order."""
        return self.min_speech, self.min_silence, self.max_frames, self.capacity


class SegmentResult(_RecordView):
    """The segmenter's view of a batch.  int32 device tensors (B): ``frames`` (frames seen), ``speech_run`` / ``silence_run`` (the
    consecutive speech / other frames ending at the last frame; one of them is 0), ``open_start`` (the first frame of the segment that
    is open, -1: none is) and ``count`` (segments closed so far, in all).  ``ring`` (B, S, 4) int32: the closed segments ``(start, end,
    reason, 0)``, segment k of a row in entry ``k % S``; a segment is the frames ``[start, end)``, reason 0 = ended by silence, 1 =
    closed at ``max_frames``; an entry never written is ``(-1, -1, -1, 0)``.  ``dropped`` (B): the segments the ring no longer holds,
    ``max(count - S, 0)``.  Only ``spans()`` reads the device: ``bool((r.count > seen).any())`` is the caller's synchronisation.  The
    tensors are views of the state record they were made from: a stream's ``result`` shows its committed record and moves with the
    next ``push`` or ``reset()``, a peek's shows the peek record until the next ``peek``; ``clone()`` keeps one."""

    FIELDS = ('frames', 'speech_run', 'silence_run', 'open_start', 'count')
    WORDS = {name: (k, torch.int32) for k, name in enumerate(FIELDS)}       # of a record (B, 8 + 4 S) int32

    def __init__(self, state):
        super().__init__(state)
        self.capacity = (state.shape[1] - hip.SEGMENT_HEAD_WORDS) // hip.SEGMENT_ENTRY_WORDS
        self.ring = state[:, hip.SEGMENT_HEAD_WORDS:].unflatten(1, (self.capacity, hip.SEGMENT_ENTRY_WORDS))

    @property
    def dropped(self):
        return (self.count - self.capacity).clamp(min=0)

    def seconds(self):
        """(``open_start`` (B), the ring's ``start`` (B, S), the ring's ``end`` (B, S)) as float32 device tensors of seconds from the
        stream's start: a segment runs from the START of its first frame, ``start * FRAME_SECONDS``, to the END of its last, ``end *
        FRAME_SECONDS``; -1 (nothing open, an entry never written) stays -1.0."""
        return tuple(self._frame_seconds(t) for t in (self.open_start, self.ring[:, :, 0], self.ring[:, :, 1]))

    def spans(self, include_open=False):
        """The segments as host values -- the one method here that reads the device (one copy of the record).  Per row a list of
        ``(start, end, reason)`` in the order they closed: the last ``min(count, S)`` closed segments (``dropped`` older ones are gone).
        ``include_open=True`` adds a row's open segment as ``(open_start, frames, -1)``: open up to the last frame seen, the caller's to
        end there (a stream that stops mid-speech)."""
        rows = []
        for rec in self.state.cpu().tolist():
            frames, open_start, count = rec[0], rec[3], rec[4]
            kept = min(count, self.capacity)
            at = [hip.SEGMENT_HEAD_WORDS + hip.SEGMENT_ENTRY_WORDS * (k % self.capacity) for k in range(count - kept, count)]
            row = [tuple(rec[a:a + 3]) for a in at]
            if include_open and open_start >= 0:
                row.append((open_start, frames, -1))
            rows.append(row)
        return rows


def _fresh_segment_state(batch, capacity):
    """(B, 8 + 4 S) int32 on the host: the fresh rows of nbasr.h."""
    entry = [-1, -1, -1, 0]
    return torch.tensor([[0, 0, 0, -1, 0, 0, 0, 0] + entry * capacity] * batch, dtype=torch.int32)


def _segment_rules(rules, device=None):
    return _spec(rules, SegmentRules, 'rules', device)


def segment(x, output_len=None, rules=None, return_mask=False):
    """Where are the stretches of speech in these utterances?  ``x`` (B, T', C) float32 logits or log-probabilities on the device,
    ``output_len`` their valid frames (tensor, sequence or None), ``rules`` a ``SegmentRules`` (None: the defaults, 49 classes).
    Returns a ``SegmentResult`` -- with ``return_mask=True`` ``(result, mask)``, mask (B, T') uint8: 1 where the frame is speech, 0
    beyond an utterance's length.  A segment still open at an utterance's end stays open (``spans(include_open=True)``).  A fresh
    state and one step of the kernel the streams run (nbasr_ctc_segment_step): the same bits as any chunking of the frames."""
    rules = _segment_rules(rules)
    x, (b, n, _), lengths, state = _whole_utterances(x, output_len, rules, hip.ctc_segment_state_words(rules.capacity))
    mask = torch.empty(b, n, dtype=torch.uint8, device=x.device) if return_mask else None
    if b:
        hip.ctc_segment_step(x, lengths, None, state, *rules.counts, rules.speech_lo, rules.speech_hi, rules.margin, mask)
    return (SegmentResult(state), mask) if return_mask else SegmentResult(state)


class SegmentStream(_LogitDetectorStream):
    """``segment`` fed chunk by chunk, for as long as the stream lasts (nbasr_ctc_segment_step with a carried state; DESIGN.md §9
    "Segments").

        sg = SegmentStream(batch, rules, device=dev)
        r = sg.push(logits_chunk, lengths=None)  # SegmentResult of everything pushed: == segment(all frames), bit for bit
        r = sg.peek(next_chunk)                  # what push(next_chunk) would return; the stream stays as it was
        r.spans()                                # per row [(start, end, reason), ...]: the one read of the device
        sg.result                                # the committed result; sg.reset() starts new streams

    The contract is ``EndpointStream``'s: both are ``_LogitDetectorStream``s, and this class adds only its record and its launch.
    Nothing latches, so there is nothing to reset between utterances: ``count`` tells a listener how many segments have closed, the
    ring holds the last ``capacity`` of them."""

    RESULT = SegmentResult

    def __init__(self, batch, rules=None, device=None):
        batch, self.rules = _positive(batch), _segment_rules(rules, device)
        super().__init__(batch, self.rules, device)

    def _fresh_rows(self):
        return _fresh_segment_state(self.batch, self.rules.capacity)

    def _step(self, x, chunk_lengths, state_out):
        r = self.rules
        hip.ctc_segment_step(x, chunk_lengths, None if self._fresh else self.state, state_out, *r.counts, r.speech_lo, r.speech_hi, r.margin)


class KeywordSet(_DeviceTables):
    """The phrases a spotter listens for: 1 to 64 keywords, each a sequence of 1 to 32 token ids in ``[0, classes)`` without the blank,
    and one threshold per keyword.  A keyword's score at a frame is the log-likelihood ratio between the best CTC path that spells it
    and ends at that frame (starting anywhere) and the unconstrained best path over the same frames: <= 0, and 0 exactly when the greedy
    path over that span collapses to the keyword.  The first frame whose score is >= the threshold is the keyword's hit.

    ``thresholds``: one finite float <= 0 per keyword, or one for all; None gives keyword k ``-per_token * len(keyword k)``.  That
    default (one nat per token) is UNTUNED for this model: a starting point, not a recommendation.

    Validates what the C side cannot see (``ValueError``): the counts above, a token outside ``[0, classes)`` or equal to the blank, a
    threshold that is positive, NaN or infinite, a device that is not a HIP device.  Owns the device tables (tokens (K, 32) int32 with -1
    past a keyword's end, token counts, thresholds), made once, by the first step that needs them (``device`` None: the current HIP
    device)."""

    OWNER, THINGS, SHOWN = 'the keyword spotter', 'the keywords', ('keywords', 'thresholds', 'classes', 'blank')

    def __init__(self, keywords, thresholds=None, per_token=1.0, classes=49, blank=0, device=None):
        classes, blank = _class_count(classes, blank)
        if isinstance(keywords, (str, bytes)) or not hasattr(keywords, '__iter__'):
            raise ValueError('keywords must be a sequence of token-id sequences')
        words = []
        for word in keywords:
            if isinstance(word, (str, bytes)) or not hasattr(word, '__iter__'):
                raise ValueError(f'a keyword is a sequence of token ids (got {word!r}); names go through KeywordSet.from_phonemes')
            word = list(word.tolist() if isinstance(word, torch.Tensor) else word)
            if any(isinstance(t, (bool, str, bytes)) or int(t) != t for t in word):
                raise ValueError(f'a keyword is a sequence of token ids (got {word})')
            words.append(tuple(int(t) for t in word))
        if not 1 <= len(words) <= MAX_KEYWORDS:
            raise ValueError(f'there must be 1 to {MAX_KEYWORDS} keywords (got {len(words)})')
        for word in words:
            if not 1 <= len(word) <= MAX_KEYWORD_TOKENS:
                raise ValueError(f'a keyword has 1 to {MAX_KEYWORD_TOKENS} tokens (got {len(word)})')
            for t in word:
                if not 0 <= t < classes:
                    raise ValueError(f'a token must lie in [0, {classes}) (got {t})')
                if t == blank:
                    raise ValueError(f'a keyword cannot hold the blank ({blank})')
        if thresholds is None:
            per_token = float(per_token)
            if not 0.0 <= per_token < float('inf'):
                raise ValueError(f'per_token must be a finite number >= 0 (got {per_token})')
            thresholds = [-per_token * len(word) for word in words]
        elif not hasattr(thresholds, '__iter__'):
            thresholds = [thresholds] * len(words)
        thresholds = [float(t) for t in (thresholds.tolist() if isinstance(thresholds, torch.Tensor) else thresholds)]
        if len(thresholds) != len(words):
            raise ValueError(f'expected {len(words)} thresholds, got {len(thresholds)}')
        thresholds = torch.tensor(thresholds, dtype=torch.float32)          # what the kernel compares with: float32
        if not bool((torch.isfinite(thresholds) & (thresholds <= 0)).all()):
            raise ValueError(f'a threshold must be a finite number <= 0 (got {thresholds.tolist()})')
        self.keywords, self.thresholds, self.classes, self.blank = tuple(words), tuple(thresholds.tolist()), classes, blank
        self._set_device(device)

    @classmethod
    def from_phonemes(cls, keywords, thresholds=None, per_token=1.0, device=None):
        """Keywords given as phoneme names of the 48-set, ``[['sh', 'iy'], ...]``: each name's index in
        ``phonemes.vocab(48, inc_blank=True)`` (49 classes, blank 0)."""
        from ..phonemes import vocab
        index = {name: i for i, name in enumerate(vocab(48, inc_blank=True))}
        words = []
        for word in keywords:
            if isinstance(word, (str, bytes)):
                raise ValueError(f'a keyword is a sequence of phoneme names (got {word!r})')
            for name in word:
                if name not in index or index[name] == 0:
                    raise ValueError(f'{name!r} is not a phoneme of the 48-set')
            words.append([index[name] for name in word])
        return cls(words, thresholds, per_token, classes=len(index), blank=0, device=device)

    def __len__(self):
        return len(self.keywords)

    def host_tables(self):
        """(tokens (K, 32) int32 with -1 past a keyword's end, token counts (K) int32, thresholds (K) float32) on the host."""
        tokens = torch.full((len(self.keywords), MAX_KEYWORD_TOKENS), -1, dtype=torch.int32)
        for k, word in enumerate(self.keywords):
            tokens[k, :len(word)] = torch.tensor(word, dtype=torch.int32)
        counts = torch.tensor([len(word) for word in self.keywords], dtype=torch.int32)
        return tokens, counts, torch.tensor(self.thresholds, dtype=torch.float32)

    def _build(self, device):
        return tuple(t.to(device).contiguous() for t in self.host_tables())

    def tables_on(self, device):
        """The three tables on ``device``, made by the first call; a keyword set lives on one device."""
        return self._on(device)

    @property
    def tables(self):
        """The device tables (``device`` None or without an index: on the current HIP device)."""
        return self._here()


class KeywordResult(_RecordView):
    """The spotter's view of a batch: (B, K) device tensors, one entry per utterance and keyword.  int32 ``frames`` (frames seen),
    ``hit_frame`` / ``hit_start`` (the first frame whose score reached the threshold and the frame the path that ends there started at;
    -1: no hit yet), ``best_frame`` / ``best_start`` (the same for the highest score so far; the earliest frame on a tie), float32
    ``hit_score`` / ``best_score`` (-inf: none), and ``detected`` (bool, ``hit_frame >= 0``, computed on the device when asked for).
    Nothing here reads the device: ``bool(r.detected.any())`` is the caller's synchronisation.  The tensors are views of the state
    record they were made from: a stream's ``result`` shows its committed record and moves with the next ``push`` or ``reset()``, a
    peek's shows the peek record until the next ``peek``; ``clone()`` keeps one."""

    FIELDS = ('frames', 'hit_frame', 'hit_start', 'hit_score', 'best_frame', 'best_start', 'best_score')
    WORDS = {name: (k, torch.float32 if name.endswith('_score') else torch.int32) for k, name in enumerate(FIELDS)}

    @property
    def detected(self):
        return self.hit_frame >= 0

    def seconds(self):
        """(``hit_start``, ``hit_end``, ``best_start``, ``best_end``) as float32 device tensors of seconds from the utterance's start:
        a span runs from the START of its first frame, ``start * FRAME_SECONDS``, to the END of its last, ``(frame + 1) *
        FRAME_SECONDS``; where there is no hit (no frame yet) both are -1.0."""
        def span(first, last):
            return self._frame_seconds(first, last), self._frame_seconds(last + 1, last)
        return span(self.hit_start, self.hit_frame) + span(self.best_start, self.best_frame)


def _fresh_keyword_state(batch, n_keywords):
    """(B, K, 136) int32 on the host: the fresh rows of nbasr.h."""
    row = torch.full((hip.KEYWORD_STATE_WORDS,), -1, dtype=torch.int32)
    row[0] = row[7] = 0
    row[3] = row[6] = _NEG_INF_BITS
    row[8:72] = _NEG_INF_BITS
    return row.repeat(batch, n_keywords, 1)


def spot_keywords(x, output_len=None, keywords=None, return_trace=False):
    """Were these phrases said, and where?  ``x`` (B, T', C) float32 logits or log-probabilities on the device, ``output_len`` their
    valid frames (tensor, sequence or None), ``keywords`` a ``KeywordSet``.  Returns a ``KeywordResult`` -- with ``return_trace=True``
    ``(result, scores, starts)``, (B, K, T') float32 / int32: every frame's score and the frame its path started at, -inf and -1 beyond
    an utterance's length (several occurrences of a keyword show as several peaks).  A fresh state and one step of the kernel the
    streams run (nbasr_ctc_keyword_step): the same bits as any chunking of the frames."""
    if keywords is None:
        raise ValueError('keywords must be a KeywordSet: there is no default phrase')
    keywords = _spec(keywords, KeywordSet, 'keywords', default=False)
    k = len(keywords)
    x, (b, n, _), lengths, state = _whole_utterances(x, output_len, keywords, k, hip.KEYWORD_STATE_WORDS)
    scores = torch.empty(b, k, n, dtype=torch.float32, device=x.device) if return_trace else None
    starts = torch.empty(b, k, n, dtype=torch.int32, device=x.device) if return_trace else None
    if b:
        hip.ctc_keyword_step(x, lengths, *keywords.tables_on(x.device), keywords.blank, None, state, scores, starts)
    return (KeywordResult(state), scores, starts) if return_trace else KeywordResult(state)


class KeywordStream(_LogitDetectorStream):
    """``spot_keywords`` fed chunk by chunk (nbasr_ctc_keyword_step with a carried state; DESIGN.md §9 "Keywords").

        kw = KeywordStream(batch, keywords, device=dev)
        r = kw.push(logits_chunk, lengths=None)  # KeywordResult of everything pushed: == spot_keywords(all frames), bit for bit
        r = kw.peek(next_chunk)                  # what push(next_chunk) would return; the stream stays as it was
        kw.result                                # the committed result; kw.reset() starts the next utterances

    The contract is ``EndpointStream``'s: both are ``_LogitDetectorStream``s, and this class adds only its record and its launch."""

    RESULT = KeywordResult

    def __init__(self, batch, keywords, device=None):
        batch, self.keywords = _positive(batch), _spec(keywords, KeywordSet, 'keywords', default=False)
        super().__init__(batch, keywords, device)

    def _fresh_rows(self):
        return _fresh_keyword_state(self.batch, len(self.keywords))

    def _step(self, x, chunk_lengths, state_out):
        tokens, counts, thresholds = self._tables
        hip.ctc_keyword_step(x, chunk_lengths, tokens, counts, thresholds, self.keywords.blank, None if self._fresh else self.state, state_out)
