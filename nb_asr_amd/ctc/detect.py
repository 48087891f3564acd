"""Detectors over the logits: what the endpointer, the segmenter, the keyword spotter and the confidence estimator share."""
import torch

from . import FRAME_SECONDS, _chunk_rows, _lengths

NON_SPEECH_PHONEMES = ('sil', 'cl', 'vcl', 'epi')        # of the 48-set: silence, the two closures, the epenthetic silence
MAX_ENDPOINT_CLASSES = 128


def _whole(v, below=None):
    """Is ``v`` a whole number (an int or a float that holds one, never a bool) -- with ``below``, one of [0, below)?"""
    return not isinstance(v, bool) and int(v) == v and (below is None or 0 <= int(v) < below)


def _class_count(classes, blank=None):
    """``classes`` as an int, within what the detectors' kernels take; with a ``blank``, ``(classes, blank)``, the blank one of the classes."""
    classes, blank = int(classes), None if blank is None else int(blank)
    if not 2 <= classes <= MAX_ENDPOINT_CLASSES:
        raise ValueError(f'classes must lie in [2, {MAX_ENDPOINT_CLASSES}] (got {classes})')
    if blank is not None and not 0 <= blank < classes:
        raise ValueError(f'blank must lie in [0, {classes}) (got {blank})')
    return classes if blank is None else (classes, blank)


def _spec(spec, cls, noun, device=None, default=True):
    """``spec`` if it is a ``cls``, else ``ValueError`` with the caller's ``noun``; with ``default``, None is ``cls(device=device)``."""
    if spec is None and default:
        spec = cls(device=device)
    if not isinstance(spec, cls):
        raise ValueError(f"{noun} must be {'an' if cls.__name__[0] in 'AEIOU' else 'a'} {cls.__name__} (got {type(spec).__name__})")
    return spec


class _RecordView:
    """A result that reads one int32 state record: ``state`` and, per entry of a subclass's ``WORDS`` (name -> (word of the record's last
    dimension, torch.int32 or torch.float32: how to read it)), an attribute that is a view of that word, never a copy; ``FIELDS``: what ``__repr__`` shows."""

    def __init__(self, state):
        self.state = state
        views = {state.dtype: state}
        for name, (word, dtype) in self.WORDS.items():
            if dtype not in views:
                views[dtype] = state.view(dtype)
            setattr(self, name, views[dtype][..., word])

    def clone(self):
        """A copy that no later step changes (one device copy)."""
        return type(self)(self.state.clone())

    @staticmethod
    def _frame_seconds(t, valid=None):
        """Frame indices -> float32 seconds, ``t * FRAME_SECONDS``; -1.0 where ``valid`` (None: ``t`` itself) is negative."""
        return torch.where((t if valid is None else valid) >= 0, t.to(torch.float32) * FRAME_SECONDS, -1.0)

    def __repr__(self):
        return f'{type(self).__name__}(' + ', '.join(f'{name}={getattr(self, name).tolist()}' for name in self.FIELDS) + ')'


def _whole_utterances(x, output_len, spec, *record):
    """How the whole-utterance functions open -> (``x`` checked as a chunk for ``spec``, its shape, its lengths on its device, an empty (B, *record) state)."""
    x = _logit_chunk(x, spec.classes, spec.THINGS)
    return x, x.shape, _lengths(output_len, x.shape[0], x.device), torch.empty(x.shape[0], *record, dtype=torch.int32, device=x.device)


class _DeviceTables:
    """What a detector decides with (``EndpointRules``, ``KeywordSet``, ``SegmentRules``, ``ConfidenceRules``) owns its device tables, ``_build(device)``'s,
    made once.  A spec whose step takes everything by value leaves ``_build`` None: it has no tables, and ``_on`` gives None.
    ``OWNER`` / ``THINGS``: the nouns of the refusals ('the endpointer' / 'the rules'); ``SHOWN``: the attributes ``__repr__`` shows."""

    _build = None

    def __repr__(self):
        return f'{type(self).__name__}(' + ', '.join(f'{name}={getattr(self, name)!r}' for name in self.SHOWN) + ')'

    def _set_device(self, device):
        self.device = None if device is None else torch.device(device)
        if self.device is not None and self.device.type != 'cuda':
            raise ValueError(f'{self.OWNER} runs on a HIP device (got {self.device}); this package has no CPU path')
        self._built = None

    def _on(self, device):
        if self.device is not None and self.device.index is not None and self.device != device:
            raise ValueError(f'{self.THINGS} live on {self.device}, not on {device}')
        if self._build is None:
            return None
        if self._built is None:
            self.device, self._built = device, self._build(device)
        return self._built

    def _here(self):
        own = self.device is not None and self.device.index is not None
        return self._on(self.device if own else torch.device('cuda', torch.cuda.current_device()))


def _logit_chunk(x, classes, owner, batch=None):
    """Is ``x`` a chunk a detector can step over -- (``batch`` or any B, frames, ``classes``) float32 on a HIP device?  -> ``x``, contiguous.
    ``owner``: who wants ``classes`` classes ('the rules' / 'the keywords')."""
    shape = x.shape if isinstance(x, torch.Tensor) else ()
    if len(shape) != 3 or (batch is not None and shape[0] != batch):
        raise ValueError(f'expected ({"batch" if batch is None else batch}, frames, classes) logits or log-probabilities, got '
                         f'{tuple(getattr(x, "shape", ()))}')
    if shape[2] != classes:
        raise ValueError(f'{owner} are for {classes} classes, x has {shape[2]}')
    if x.dtype != torch.float32 or not x.is_cuda:
        raise ValueError(f'x must be float32 on a HIP device (got {x.dtype} on {x.device}); this package has no CPU path')
    return x.contiguous()


class _LogitDetectorStream:
    """A detector fed the logits chunk by chunk: the push / peek / reset contract of ``EndpointStream``, ``KeywordStream`` and
    ``SegmentStream`` (``ConfidenceStream`` keeps the records, the lengths and ``reset()``, and steps in its own way).

    The state is one int32 record per batch, three times: ``state``, the committed one; ``_fresh_state``, constant, what ``result``
    shows until the first frame; ``_peek_state``, which the first peek allocates and every peek overwrites.  ``reset()`` launches
    nothing: the next step is handed no input state (``state_in == NULL``) and starts from fresh rows.  A subclass gives ``RESULT``
    (the class that reads a record), ``_fresh_rows()`` (the fresh record on the host; its shape is the record's) and ``_step(x,
    chunk_lengths, state_out)``, one launch from ``None if self._fresh else self.state``; it has checked ``spec``, its rules or keywords."""

    def __init__(self, batch, spec, device):
        device = torch.device(spec.device if device is None and spec.device is not None else 'cuda' if device is None else device)
        if device.type != 'cuda':
            raise ValueError(f'{spec.OWNER} runs on a HIP device (got {device}); this package has no CPU path')
        self.device = device if device.index is not None else torch.device('cuda', torch.cuda.current_device())
        self.batch, self._tables, self._classes, self._things = batch, spec._on(self.device), spec.classes, spec.THINGS
        self._fresh_state = self._fresh_rows().to(self.device)        # never written
        self.state = torch.empty_like(self._fresh_state)
        self._peek_state = None
        self.reset()

    @property
    def state_bytes(self):
        """Device bytes of the state: the committed record, the constant fresh one, and the peek record once it exists."""
        return sum(t.numel() * t.element_size() for t in (self.state, self._fresh_state, self._peek_state) if t is not None)

    def reset(self):
        """Start a new batch of utterances.  No launch: the next step starts from fresh rows."""
        self._fresh = True
        self.ended = torch.zeros(self.batch, dtype=torch.bool)

    @property
    def result(self):
        """The result (``RESULT``) of the frames committed so far."""
        return self.RESULT(self._fresh_state if self._fresh else self.state)

    def _chunk(self, x, lengths):
        x = _logit_chunk(x, self._classes, self._things, self.batch)
        if x.device != self.device:
            raise ValueError(f'x must be on {self.device} (got {x.device})')
        n = x.shape[1]
        if lengths is None:
            return x, n, None, None
        rows = _chunk_rows(lengths, n, self.batch, self.ended)
        return x, n, rows, rows.to(device=self.device, dtype=torch.int32)

    def push(self, x, lengths=None):
        """Take the next chunk (B, n, C) of logits or log-probabilities; returns the result of everything pushed."""
        x, n, rows, chunk_lengths = self._chunk(x, lengths)
        if n:
            self._step(x, chunk_lengths, self.state)
            self._fresh = False
            if rows is not None:
                self.ended |= rows < n
        return self.result

    def peek(self, x=None, lengths=None):
        """The result ``push(x, lengths)`` would return, with the stream left as it was (the committed record is only read).  ``x`` None
        or of no frames: ``result``, no launch."""
        if x is None:
            return self.result
        x, n, _, chunk_lengths = self._chunk(x, lengths)
        if not n:
            return self.result
        if self._peek_state is None:
            self._peek_state = torch.empty_like(self.state)
        self._step(x, chunk_lengths, self._peek_state)
        return self.RESULT(self._peek_state)


def default_speech_classes():
    """The classes that count as speech for the model's 49 outputs: every class except the blank (0) and the 48-set's ``sil``, ``cl``,
    ``vcl`` and ``epi`` -- indices 0, 10, 17, 38 and 44 of ``phonemes.vocab(48, inc_blank=True)``.  A sorted tuple of ints."""
    from ..phonemes import vocab
    return tuple(i for i, name in enumerate(vocab(48, inc_blank=True)) if i != 0 and name not in NON_SPEECH_PHONEMES)


class _SpeechDecision(_DeviceTables):
    """The per-frame speech decision ``EndpointRules`` and ``SegmentRules`` share: ``classes``, the sorted ``speech_classes``, ``margin``
    and the class mask's two 64-bit words ``speech_lo`` / ``speech_hi``, validated as the C side does (``ValueError``)."""

    def _set_speech(self, speech_classes, margin, classes):
        classes = _class_count(classes)
        if speech_classes is None:
            if classes != 49:
                raise ValueError(f'speech_classes must be given for {classes} classes (the default is for the 48-set and the blank)')
            speech_classes = default_speech_classes()
        given = [int(c) for c in speech_classes]
        speech = sorted(set(given))
        if len(speech) != len(given):
            raise ValueError('speech_classes names a class twice')
        if not speech:
            raise ValueError('speech_classes is empty')
        if speech[0] < 0 or speech[-1] >= classes:
            raise ValueError(f'speech_classes must lie in [0, {classes}) (got {speech[0]}..{speech[-1]})')
        if len(speech) == classes:
            raise ValueError('speech_classes is every class: no class is left for non-speech')
        margin = float(margin)
        if not margin >= 0.0:
            raise ValueError(f'margin must be a number >= 0 (got {margin})')
        self.speech_classes, self.margin, self.classes = tuple(speech), margin, classes
        word = sum(1 << c for c in speech)
        self.speech_lo, self.speech_hi = word & (2 ** 64 - 1), word >> 64
