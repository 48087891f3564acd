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
import collections
import inspect

import torch

from . import hip
from .frontend import LogMelFrontend
from .phonemes import fold_table  # noqa: F401  (part of this module's interface)

OUTPUT_STRIDE = 4                 # input frames per output frame: the model's two stride-2 convolutions
_FRONTEND = inspect.signature(LogMelFrontend.__init__).parameters
# seconds per output frame: the front-end's hop (160 samples at 16 kHz = 10 ms) times the model's stride = 40 ms; turns frame spans into seconds
FRAME_SECONDS = OUTPUT_STRIDE * _FRONTEND['hop_length'].default / _FRONTEND['sample_rate'].default


def output_lengths(audio_len):
    """Frames of the model output that belong to each utterance: ``audio_len // 4`` (trainer.py:219).  Note this is the
    trainer's convention, not ceil(ceil(T/2)/2): for T not divisible by 4 the last partial output frame is ignored."""
    return torch.div(audio_len, OUTPUT_STRIDE, rounding_mode='floor')


def log_softmax(logits):
    """(B, T', C) float32 on a HIP device -> log-probabilities, same shape."""
    return hip.ctc_postprocess(logits, None, True, False)[0]


def greedy_decode(logits, audio_len=None, blank=0, return_log_probs=False):
    """Greedy CTC decoding of model logits.

    ``audio_len``: per-utterance input lengths in frames (tensor or sequence); outputs beyond ``audio_len // 4`` are ignored.
    Returns a list of 1-D int32 CPU tensors (one token sequence per utterance), plus the log-probabilities if requested."""
    lengths = None
    if audio_len is not None:
        lengths = output_lengths(torch.as_tensor(audio_len)).to(device=logits.device, dtype=torch.int32).contiguous()
    log_probs, tokens, counts = hip.ctc_postprocess(logits.contiguous(), lengths, return_log_probs, True, blank)
    tokens, counts = tokens.cpu(), counts.cpu()
    seqs = [tokens[i, : int(counts[i])] for i in range(tokens.shape[0])]
    return (seqs, log_probs) if return_log_probs else seqs


def _lengths(lengths, batch, device):
    if lengths is None:
        return None
    lengths = torch.as_tensor(lengths)
    if lengths.numel() != batch:
        raise ValueError(f'expected {batch} lengths, got {lengths.numel()}')
    return lengths.to(device=device, dtype=torch.int32).contiguous()


def bigram_lm(targets, targets_len, classes=49, blank=0, smoothing=1.0):
    """The classical LM of a phoneme recogniser: a bigram estimated from transcripts.  ``targets`` (N, L) integer labels with their lengths
    ``targets_len`` (N) (tensors or sequences; labels beyond a length are ignored, ``blank`` is never a label).  Returns a (classes, classes)
    float32 tensor of ``log P(c | prev)`` on ``targets``' device, from add-``smoothing`` counts over the non-blank classes:
    ``(count(prev, c) + smoothing) / (count(prev, .) + smoothing * (classes - 1))``.  Row ``blank`` is the distribution of first tokens (the
    context of the empty prefix); column ``blank`` is filled with its row's minimum (a finite value; the search never reads it).
    Plain torch, any device."""
    targets = torch.as_tensor(targets).to(torch.int64)
    if targets.dim() != 2:
        raise ValueError(f'targets must be (transcripts, labels), got {tuple(targets.shape)}')
    n, width = targets.shape
    lens = torch.as_tensor(targets_len).to(device=targets.device, dtype=torch.int64).reshape(-1)
    if lens.numel() != n:
        raise ValueError(f'expected {n} lengths, got {lens.numel()}')
    valid = torch.arange(width, device=targets.device)[None, :] < lens.clamp(0, width)[:, None]
    if bool(((targets[valid] < 0) | (targets[valid] >= classes) | (targets[valid] == blank)).any()):
        raise ValueError(f'labels must lie in [0, {classes}) and differ from blank={blank}')
    prev = torch.cat([torch.full((n, 1), blank, dtype=torch.int64, device=targets.device), targets[:, :-1]], 1)
    counts = torch.zeros(classes * classes, dtype=torch.float64, device=targets.device)
    counts.index_add_(0, (prev * classes + targets)[valid], torch.ones(int(valid.sum()), dtype=torch.float64, device=targets.device))
    counts = counts.view(classes, classes) + float(smoothing)
    counts[:, blank] = 0.0
    lm = torch.log(counts / counts.sum(1, keepdim=True))
    lm[:, blank] = float('inf')
    lm[:, blank] = lm.min(1).values
    return lm.to(torch.float32)


def fusion_table(lm, alpha=1.0, beta=0.0, device=None):
    """The table the fused searches add (nbasr.h "bigram LM fusion"): ``W = alpha * lm + beta`` in float32, contiguous, on ``device``
    (None: where ``lm`` is).  ``lm``: (C, C) ``log P(c | prev)`` with row ``blank`` for the start of an utterance, e.g. ``bigram_lm``;
    ``alpha`` weighs the LM, ``beta`` is added per token (ctcdecode's alpha / beta).  Raises ``ValueError`` for anything but a square
    matrix of at most 64 classes or for entries that are not finite: the one place that validates a table."""
    lm = torch.as_tensor(lm)
    if lm.dim() != 2 or lm.shape[0] != lm.shape[1] or not 1 <= lm.shape[0] <= 64:
        raise ValueError(f'lm must be (classes, classes) with at most 64 classes, got {tuple(lm.shape)}')
    table = lm.to(torch.float32) * torch.tensor(alpha, dtype=torch.float32) + torch.tensor(beta, dtype=torch.float32)
    if not bool(torch.isfinite(table).all()):
        raise ValueError('every entry of alpha * lm + beta must be finite (a forbidden transition is not supported)')
    return table.to(device=lm.device if device is None else device).contiguous()


def _fusion(lm, alpha, beta, classes, device):
    """None without an LM, else the fusion table for a search over ``classes`` classes on ``device``."""
    if lm is None:
        return None
    table = fusion_table(lm, alpha, beta, device)
    if classes is not None and table.shape[0] != classes:
        raise ValueError(f'lm has {table.shape[0]} classes, the log-probabilities {classes}')
    return table


def beam_decode(log_probs, output_len=None, beam_width=12, blank=0, cutoff_top_n=40, *, return_timesteps=False, lm=None, alpha=1.0, beta=0.0):
    """CTC prefix beam search over log-probabilities (B, T', C), the reference's
    ``CTCBeamDecoder(vocab, beam_width=12, log_probs_input=True).decode(output, output_len)`` (trainer.py:71,237).

    ``output_len``: valid output frames per utterance (``output_lengths(audio_len)``), tensor or sequence, or None.
    Returns ``(beams, scores, out_len)`` on the device: beams (B, beam_width, T') int32 best first (entries beyond ``out_len``
    are 0), scores (B, beam_width) = -log P (lower is better), out_len (B, beam_width) int32.  ``return_timesteps=True`` returns
    ctcdecode's four outputs in its order, ``(beams, scores, timesteps, out_len)``: timesteps (B, beam_width, T') int32, for
    every token the frame at which its class was most probable among the frames that extended into it (DESIGN.md §9 "Beam
    decode"; 0 beyond ``out_len``).  The search is the same one, bit for bit.

    ``lm``: a (C, C) matrix of ``log P(c | previous token)`` (``bigram_lm``; row ``blank`` = start of the utterance) fused into the search
    as ctcdecode's scorer is: every extension of a prefix ending in p by class c adds ``alpha * lm[p][c] + beta`` to the log score
    (``fusion_table``; DESIGN.md §9 "Beam decode").  ``scores`` are then minus the fused log score.  None: no LM, today's search."""
    if log_probs.dim() != 3:
        raise ValueError(f'log_probs must be (batch, frames, classes), got {tuple(log_probs.shape)}')
    lengths = _lengths(output_len, log_probs.shape[0], log_probs.device)
    return hip.ctc_beam_search(log_probs.contiguous(), lengths, beam_width, blank, cutoff_top_n, timesteps=bool(return_timesteps),
                               fusion=_fusion(lm, alpha, beta, log_probs.shape[2], log_probs.device))


def _cut_rows(host, at, n_c, counts):
    """One track of a step's rows on the host, its committed rows from column ``at`` and its partial rows ``n_c`` columns on, cut into
    per-utterance tensors by ``counts`` = (committed counts, partial counts, ...) -> (committed rows, partial rows)."""
    batch = range(host.shape[0])
    return ([host[i, at: at + int(counts[0, i])].clone() for i in batch],
            [host[i, at + n_c: at + n_c + int(counts[1, i])].clone() for i in batch])


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


class BeamSearchStream:
    """``beam_decode`` fed chunk by chunk, with committed partial results (nbasr_ctc_beam_stream_*; DESIGN.md §9 "Beam decode").

        dec = BeamSearchStream(batch, beam_width=12, blank=0, cutoff_top_n=40, device=dev)
        committed, partial = dec.push(log_probs_chunk, lengths=None)   # lists of int32 CPU tensors, one per utterance
        beams, scores, out_len = dec.finish()     # == beam_decode(all frames, total lengths), bit for bit
        beams, scores, out_len = dec.peek(next_chunk)                  # what finish() would give after push(next_chunk); changes nothing

    ``committed``: the tokens that became final with this chunk -- a prefix of every beam the search can still return, so they
    never change; the committed tokens of all pushes, concatenated, start every finite-score beam of ``finish()``.  ``partial``:
    the current best beam's tokens after everything committed so far.  ``lengths`` (B) gives each utterance's frames in this
    chunk; fewer than the chunk has ends that utterance, and it takes no frames after that.  The token pool of the search keeps only
    the uncommitted parts of the live beams and grows (keeping its contents) when a push could overflow it: memory depends on how
    far the beams diverge, not on the length of the stream.

    ``timesteps=True`` (``beam_decode(..., return_timesteps=True)`` fed chunk by chunk): ``push`` returns ``(committed, partial,
    committed_frames, partial_frames)`` -- lists of int32 CPU tensors aligned with the token lists, each token's frame counted per
    utterance from ``reset()`` across pushes; a committed token's frame is final -- and ``finish()`` returns
    ``(beams, scores, timesteps, out_len)``.

    ``lm``, ``alpha``, ``beta``: ``beam_decode``'s bigram fusion fed chunk by chunk.  The table is built once, here; ``push`` and ``peek``
    use it, ``reset()`` keeps it, and every chunk must have the table's classes."""

    def __init__(self, batch, beam_width=12, blank=0, cutoff_top_n=40, device=None, pool_nodes=None, timesteps=False, *, lm=None, alpha=1.0,
                 beta=0.0):
        batch, beam_width = _positive(batch), int(beam_width)
        if not 1 <= beam_width <= 32:
            raise ValueError(f'beam_width must be in [1, 32] (got {beam_width})')
        self.batch, self.beam_width, self.blank, self.cutoff_top_n = batch, beam_width, int(blank), int(cutoff_top_n)
        self.timesteps = bool(timesteps)
        device = torch.device('cuda' if device is None else device)
        if device.type != 'cuda':
            raise ValueError(f'the beam search runs on a HIP device (got {device}); this package has no CPU path')
        self.device = device if device.index is not None else torch.device('cuda', torch.cuda.current_device())
        self.initial_pool_nodes = int(pool_nodes) if pool_nodes is not None else 1 + beam_width * 4 * 40
        self.fusion = _fusion(lm, alpha, beta, None, self.device)          # the fusion table on the device, or None: no LM
        self.state = None
        self._peek_ws = None                      # peek's scratch pool, kept between peeks (reset() keeps it too)
        self.reset()

    @property
    def state_bytes(self):
        """Device bytes of the search state (live beams and token pool)."""
        return 0 if self.state is None else self.state.numel() * self.state.element_size()

    def reset(self):
        """Start a new batch of utterances at the empty prefix (the state keeps its current pool size)."""
        if self.state is None:
            self.pool_nodes = self.initial_pool_nodes
            self.state = torch.empty(self._words(self.pool_nodes), dtype=torch.int64, device=self.device)
        hip.ctc_beam_stream_init(self.state, self.batch, self.beam_width, self.pool_nodes, self.timesteps)
        self.usage = torch.ones(self.batch, dtype=torch.int64)
        self.ended = torch.zeros(self.batch, dtype=torch.bool)
        self.committed = [[] for _ in range(self.batch)]
        self.partial = [torch.zeros(0, dtype=torch.int32) for _ in range(self.batch)]
        self.committed_frames = [[] for _ in range(self.batch)]       # with timesteps: aligned with committed / partial
        self.partial_frames = [torch.zeros(0, dtype=torch.int32) for _ in range(self.batch)]
        self.frames = 0
        self.classes = None if self.fusion is None else self.fusion.shape[0]
        self.grown = 0
        self._finished = False

    def _words(self, pool_nodes):
        return (hip.ctc_beam_stream_state_bytes(self.batch, self.beam_width, pool_nodes, self.timesteps) + 7) // 8

    def _grow(self, need):
        """Enlarge the pool to at least ``need`` nodes: every utterance's record keeps its bytes at the start of its new record."""
        new_nodes = max(need, 2 * self.pool_nodes)
        old_rec = self.state.numel() // self.batch
        new = torch.empty(self._words(new_nodes), dtype=torch.int64, device=self.device)
        new.view(self.batch, -1)[:, :old_rec].copy_(self.state.view(self.batch, -1))
        self.state, self.pool_nodes = new, new_nodes
        self.grown += 1

    def _chunk(self, log_probs, lengths, empty_has_classes=True):
        """Is this a valid chunk with valid lengths for this stream?  -> (frames, classes, the utterances' frames in the chunk: int64 (B) on
        the host).  ``empty_has_classes``: a chunk of no frames must have the stream's classes too."""
        if self._finished:
            raise ValueError('push after finish(): call reset() to start the next utterances')
        if not isinstance(log_probs, torch.Tensor) or log_probs.dim() != 3 or log_probs.shape[0] != self.batch:
            raise ValueError(f'expected log-probabilities ({self.batch}, frames, classes), got {tuple(getattr(log_probs, "shape", ()))}')
        if log_probs.dtype != torch.float32 or log_probs.device != self.device:
            raise ValueError(f'log-probabilities must be float32 on {self.device} (got {log_probs.dtype} on {log_probs.device})')
        n, c = log_probs.shape[1], log_probs.shape[2]
        if self.classes is not None and c != self.classes and (n or empty_has_classes):
            raise ValueError(f'every chunk must have {self.classes} classes (got {c})')
        return n, c, _chunk_rows(lengths, n, self.batch, self.ended)

    def push(self, log_probs, lengths=None):
        """Decode the next chunk of log-probabilities (B, n, C) float32 on the device.  Returns ``(committed, partial)``, with
        ``timesteps`` ``(committed, partial, committed_frames, partial_frames)``."""
        n, c, rows = self._chunk(log_probs, lengths)
        self.classes = c
        if n == 0:
            return self._pushed([[torch.zeros(0, dtype=torch.int32) for _ in range(self.batch)] for _ in self._tracks()])
        need = int(self.usage.max()) + self.beam_width * n + 1
        if need > self.pool_nodes:
            self._grow(need)
        chunk_lengths = None if lengths is None else rows.to(device=self.device, dtype=torch.int32)
        *rows_out, counts = hip.ctc_beam_stream_step(log_probs.contiguous(), chunk_lengths, self.state, self.beam_width, self.pool_nodes,
                                                     self.blank, self.cutoff_top_n, self.timesteps, self.fusion)
        counts = counts.cpu()
        if bool((counts[2] < 0).any()):
            raise hip.HipError('ctc_beam_stream_step: the token pool was too small for the chunk')
        self.usage = counts[2].to(torch.int64)
        n_c, n_p = int(counts[0].max()), int(counts[1].max())
        # one copy for all rows: per track its committed rows cut to n_c columns, then its partial rows cut to n_p
        host = torch.cat([r[:, :k] for r, k in zip(rows_out, (n_c, n_p) * len(self._tracks()))], 1).cpu()
        new = []
        for k, (committed, partial) in enumerate(self._tracks()):
            more, now = _cut_rows(host, k * (n_c + n_p), n_c, counts)
            setattr(self, partial, now)
            for i in range(self.batch):
                getattr(self, committed)[i].append(more[i])
            new.append(more)
        self.ended |= rows < n
        self.frames += n
        return self._pushed(new)

    def _tracks(self):
        """The attributes that hold what a push cuts its rows into, (committed lists, partial list): the tokens and, with timesteps, their frames."""
        return (('committed', 'partial'), ('committed_frames', 'partial_frames'))[: 2 if self.timesteps else 1]

    def _pushed(self, new):
        """What a push returns: per track the rows committed by it (``new``), then the partial rows as they now stand."""
        return tuple(rows for more, (_, partial) in zip(new, self._tracks()) for rows in (more, list(getattr(self, partial))))

    def finish(self):
        """End the utterances: ``(beams (B, W, T) int32, scores (B, W), out_len (B, W) int32)`` on the device, ``beam_decode``'s layout
        over the T frames pushed; with ``timesteps`` ``(beams, scores, timesteps (B, W, T) int32, out_len)``."""
        if self._finished:
            raise ValueError('finish() called twice: call reset() to start the next utterances')
        self._finished = True
        ld = max(int(self.usage.max()) - 1, 1)
        return self._assemble(hip.ctc_beam_stream_finish(self.state, self.batch, self.beam_width, self.pool_nodes, ld, self.timesteps), self.frames)

    def peek(self, log_probs=None, lengths=None):
        """What ``finish()`` would return if ``push(log_probs, lengths)`` had been called first (None: no more frames), with the search left
        exactly as it was: the state is only read (nbasr_ctc_beam_stream_peek), no attribute changes, the pool never grows.  Allowed any
        number of times before ``finish()``; only the workspace (``peek_bytes``) is kept, for the next peek."""
        if log_probs is None and not self._finished:
            log_probs = torch.empty(self.batch, 0, self.classes or self.blank + 1, dtype=torch.float32, device=self.device)
        n, c, rows = self._chunk(log_probs, lengths, empty_has_classes=False)
        chunk_lengths = None if lengths is None else rows.to(device=self.device, dtype=torch.int32)
        self.reserve_peek(n, c)
        ld = max(int(self.usage.max()) - 1 + n, 1)               # a frame lengthens a suffix by at most one token
        outs = hip.ctc_beam_stream_peek(log_probs.contiguous(), chunk_lengths, self.state, self.beam_width, self.pool_nodes, ld, self.blank,
                                        self.cutoff_top_n, self.timesteps, self._peek_ws, self.fusion)
        return self._assemble(outs, self.frames + n)

    def reserve_peek(self, frames, classes=None):
        """Make the cached peek workspace large enough for peeks of up to ``frames`` frames (a caller that bounds its memory calls this
        once; ``peek`` calls it with its own chunk, so the workspace only ever grows)."""
        need = hip.ctc_beam_stream_peek_workspace_bytes(self.batch, frames, classes or self.classes or 1, self.beam_width, self.pool_nodes)
        if self._peek_ws is None or self._peek_ws.numel() * 8 < need:
            self._peek_ws = hip._scratch(need, self.device, torch.int64)

    @property
    def peek_bytes(self):
        """Device bytes of the cached peek workspace (0 before the first ``peek``); not part of ``state_bytes``."""
        return 0 if self._peek_ws is None else self._peek_ws.numel() * 8

    def _assemble(self, outs, frames):
        """Committed heads + the live suffixes of a finish / peek launch -> ``beam_decode``'s layout over ``frames`` frames."""
        suffix, scores, *suffix_t, lens = outs
        tails = [(tail.cpu(), getattr(self, heads)) for tail, (heads, _) in zip((suffix, *suffix_t), self._tracks())]
        lens = lens.cpu()
        outs = [torch.zeros(self.batch, self.beam_width, frames, dtype=torch.int32) for _ in tails]
        live = lens >= 0                                         # (B, W): beyond the live prefixes there is no beam: length 0, padded with 0
        n_c = torch.tensor([sum(c.numel() for c in self.committed[i]) for i in range(self.batch)], dtype=torch.int32)
        out_len = torch.where(live, n_c[:, None] + lens, 0).to(torch.int32)
        for (tail, heads), out in zip(tails, outs):               # the tokens, then (timed) their frames: committed head + live suffix
            for i in range(self.batch):
                at = int(n_c[i])
                if at:
                    out[i, live[i], :at] = torch.cat(heads[i])
                w = min(tail.shape[2], frames - at)               # a beam holds at most one token per frame: every suffix ends by `frames`
                keep = torch.arange(w)[None, :] < lens[i][:, None]
                out[i, :, at: at + w] = torch.where(keep, tail[i, :, :w], 0)
        beams, timesteps = [out.to(self.device) for out in outs] + [None] * (2 - len(outs))
        return hip.beam_result(beams, scores, timesteps, out_len.to(self.device))


def empty_beam_result(batch, beam_width, device, timesteps=False):
    """``BeamSearchStream.finish()`` of a search that saw no frame, without a search or a launch: the empty prefix alone, at
    -log P = -0.0; ``(beams (B, W, 0), scores, out_len)``, with ``timesteps`` ``(beams, scores, timesteps (B, W, 0), out_len)``."""
    scores = torch.full((batch, beam_width), torch.finfo(torch.float32).max)
    scores[:, 0] = -0.0
    none = torch.zeros(batch, beam_width, 0, dtype=torch.int32).to(device)
    lens = torch.zeros(batch, beam_width, dtype=torch.int32).to(device)
    return hip.beam_result(none, scores.to(device), none.clone() if timesteps else None, lens)


# ---- detectors over the logits: what the endpointer, the keyword spotter and the segmenter share ------------------------
class _DeviceTables:
    """What a detector decides with (``EndpointRules``, ``KeywordSet``, ``SegmentRules``, ``ConfidenceRules``) owns its device tables, ``_build(device)``'s,
    made once.  A spec whose step takes everything by value leaves ``_build`` None: it has no tables, and ``_on`` gives None.
    ``OWNER`` / ``THINGS``: the nouns of the refusals ('the endpointer' / 'the rules')."""

    _build = None

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


# ---- endpointing: when has an utterance ended? (nbasr.h "endpointing"; DESIGN.md §9 "Endpoint") ---------------------------------------
NON_SPEECH_PHONEMES = ('sil', 'cl', 'vcl', 'epi')        # of the 48-set: silence, the two closures, the epenthetic silence
MAX_ENDPOINT_RULES = 8
MAX_ENDPOINT_CLASSES = 128


def default_speech_classes():
    """The classes that count as speech for the model's 49 outputs: every class except the blank (0) and the 48-set's ``sil``, ``cl``,
    ``vcl`` and ``epi`` -- indices 0, 10, 17, 38 and 44 of ``phonemes.vocab(48, inc_blank=True)``.  A sorted tuple of ints."""
    from .phonemes import vocab
    return tuple(i for i, name in enumerate(vocab(48, inc_blank=True)) if i != 0 and name not in NON_SPEECH_PHONEMES)


class _SpeechDecision(_DeviceTables):
    """The per-frame speech decision ``EndpointRules`` and ``SegmentRules`` share: ``classes``, the sorted ``speech_classes``, ``margin``
    and the class mask's two 64-bit words ``speech_lo`` / ``speech_hi``, validated as the C side does (``ValueError``)."""

    def _set_speech(self, speech_classes, margin, classes):
        classes = int(classes)
        if not 2 <= classes <= MAX_ENDPOINT_CLASSES:
            raise ValueError(f'classes must lie in [2, {MAX_ENDPOINT_CLASSES}] (got {classes})')
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

    OWNER, THINGS = 'the endpointer', 'the rules'

    def __init__(self, rules=((0, 125, 0), (1, 25, 0), (0, 0, 500)), speech_classes=None, margin=0.0, classes=49, device=None):
        self._set_speech(speech_classes, margin, classes)
        rules = tuple(tuple(rule) for rule in rules)
        if not 1 <= len(rules) <= MAX_ENDPOINT_RULES:
            raise ValueError(f'there must be 1 to {MAX_ENDPOINT_RULES} rules (got {len(rules)})')
        for rule in rules:
            if len(rule) != 3 or any(isinstance(v, bool) or int(v) != v or not 0 <= int(v) < 2 ** 31 for v in rule):
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

    def __repr__(self):
        return f'EndpointRules(rules={self.rules}, speech_classes={self.speech_classes}, margin={self.margin}, classes={self.classes})'


class EndpointResult:
    """The endpointer's view of a batch: int32 device tensors (B) ``frames`` (frames seen), ``speech_frames``, ``first_speech`` and
    ``last_speech`` (frame indices, -1: none yet), ``endpoint_frame`` (the frame at which the first rule held, -1: no endpoint yet)
    and ``rule`` (that rule's index, -1).  Nothing here reads the device: ``bool((r.endpoint_frame >= 0).any())`` is the caller's
    synchronisation.  The tensors are columns of the state record they were made from: a stream's ``result`` shows its committed
    record and moves with the next ``push`` or ``reset()``, a peek's shows the peek record until the next ``peek``; ``clone()`` keeps one."""

    FIELDS = ('frames', 'speech_frames', 'first_speech', 'last_speech', 'endpoint_frame', 'rule')

    def __init__(self, state):
        self.state = state                       # (B, 8) int32
        for k, name in enumerate(self.FIELDS):
            setattr(self, name, state[:, k])

    def clone(self):
        """A copy that no later step changes (one device copy)."""
        return EndpointResult(self.state.clone())

    def seconds(self):
        """(``endpoint_frame``, ``first_speech``, ``last_speech``) as float32 device tensors of seconds from the utterance's start:
        the START of each frame, ``frame * FRAME_SECONDS``; -1 frames stay -1.0."""
        return tuple(torch.where(t >= 0, t.to(torch.float32) * FRAME_SECONDS, -1.0) for t in (self.endpoint_frame, self.first_speech, self.last_speech))

    def __repr__(self):
        return 'EndpointResult(' + ', '.join(f'{name}={getattr(self, name).tolist()}' for name in self.FIELDS) + ')'


def endpoint(x, output_len=None, rules=None, return_mask=False):
    """Where do these utterances end?  ``x`` (B, T', C) float32 logits or log-probabilities on the device, ``output_len`` their valid
    frames (tensor, sequence or None), ``rules`` an ``EndpointRules`` (None: the defaults, 49 classes).  Returns an ``EndpointResult``
    -- with ``return_mask=True`` ``(result, mask)``, mask (B, T') uint8: 1 where the frame is speech, 0 beyond an utterance's length.
    A fresh state and one step of the kernel the streams run (nbasr_ctc_endpoint_step): the same bits as any chunking of the frames."""
    rules = EndpointRules() if rules is None else rules
    if not isinstance(rules, EndpointRules):
        raise ValueError(f'rules must be an EndpointRules (got {type(rules).__name__})')
    x = _logit_chunk(x, rules.classes, rules.THINGS)
    b, n, _ = x.shape
    lengths = _lengths(output_len, b, x.device)
    state = torch.empty(b, hip.ENDPOINT_STATE_WORDS, dtype=torch.int32, device=x.device)
    mask = torch.empty(b, n, dtype=torch.uint8, device=x.device) if return_mask else None
    if b:
        hip.ctc_endpoint_step(x, lengths, None, state, rules.table_on(x.device), rules.speech_lo, rules.speech_hi, rules.margin, mask)
    result = EndpointResult(state)
    return (result, mask) if return_mask else result


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
        batch = _positive(batch)
        rules = EndpointRules(device=device) if rules is None else rules
        if not isinstance(rules, EndpointRules):
            raise ValueError(f'rules must be an EndpointRules (got {type(rules).__name__})')
        self.rules = rules
        super().__init__(batch, rules, device)

    def _fresh_rows(self):
        return torch.tensor([[0, 0, -1, -1, -1, -1, 0, 0]] * self.batch, dtype=torch.int32)

    def _step(self, x, chunk_lengths, state_out):
        r = self.rules
        hip.ctc_endpoint_step(x, chunk_lengths, None if self._fresh else self.state, state_out, self._tables, r.speech_lo, r.speech_hi, r.margin)


# ---- segments: where are the stretches of speech in this stream? (nbasr.h "segmentation"; DESIGN.md §9 "Segments") --------------------
MAX_SEGMENT_CAPACITY = hip.SEGMENT_MAX_CAPACITY


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

    def __init__(self, min_speech=3, min_silence=13, max_frames=0, capacity=16, speech_classes=None, margin=0.0, classes=49, device=None):
        self._set_speech(speech_classes, margin, classes)
        for name, v in (('min_speech', min_speech), ('min_silence', min_silence), ('max_frames', max_frames), ('capacity', capacity)):
            if isinstance(v, bool) or int(v) != v or not 0 <= int(v) < 2 ** 31:
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

    def __repr__(self):
        return (f'SegmentRules(min_speech={self.min_speech}, min_silence={self.min_silence}, max_frames={self.max_frames}, '
                f'capacity={self.capacity}, speech_classes={self.speech_classes}, margin={self.margin}, classes={self.classes})')


class SegmentResult:
    """The segmenter's view of a batch.  int32 device tensors (B): ``frames`` (frames seen), ``speech_run`` / ``silence_run`` (the
    consecutive speech / other frames ending at the last frame; one of them is 0), ``open_start`` (the first frame of the segment that
    is open, -1: none is) and ``count`` (segments closed so far, in all).  ``ring`` (B, S, 4) int32: the closed segments ``(start, end,
    reason, 0)``, segment k of a row in entry ``k % S``; a segment is the frames ``[start, end)``, reason 0 = ended by silence, 1 =
    closed at ``max_frames``; an entry never written is ``(-1, -1, -1, 0)``.  ``dropped`` (B): the segments the ring no longer holds,
    ``max(count - S, 0)``.  Only ``spans()`` reads the device: ``bool((r.count > seen).any())`` is the caller's synchronisation.  The
    tensors are views of the state record they were made from: a stream's ``result`` shows its committed record and moves with the
    next ``push`` or ``reset()``, a peek's shows the peek record until the next ``peek``; ``clone()`` keeps one."""

    FIELDS = ('frames', 'speech_run', 'silence_run', 'open_start', 'count')

    def __init__(self, state):
        self.state = state                       # (B, 8 + 4 S) int32
        for k, name in enumerate(self.FIELDS):
            setattr(self, name, state[:, k])
        self.capacity = (state.shape[1] - hip.SEGMENT_HEAD_WORDS) // hip.SEGMENT_ENTRY_WORDS
        self.ring = state[:, hip.SEGMENT_HEAD_WORDS:].unflatten(1, (self.capacity, hip.SEGMENT_ENTRY_WORDS))

    @property
    def dropped(self):
        return (self.count - self.capacity).clamp(min=0)

    def clone(self):
        """A copy that no later step changes (one device copy)."""
        return SegmentResult(self.state.clone())

    def seconds(self):
        """(``open_start`` (B), the ring's ``start`` (B, S), the ring's ``end`` (B, S)) as float32 device tensors of seconds from the
        stream's start: a segment runs from the START of its first frame, ``start * FRAME_SECONDS``, to the END of its last, ``end *
        FRAME_SECONDS``; -1 (nothing open, an entry never written) stays -1.0."""
        return tuple(torch.where(t >= 0, t.to(torch.float32) * FRAME_SECONDS, -1.0) for t in (self.open_start, self.ring[:, :, 0], self.ring[:, :, 1]))

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

    def __repr__(self):
        return 'SegmentResult(' + ', '.join(f'{name}={getattr(self, name).tolist()}' for name in self.FIELDS) + ')'


def _fresh_segment_state(batch, capacity):
    """(B, 8 + 4 S) int32 on the host: the fresh rows of nbasr.h."""
    entry = [-1, -1, -1, 0]
    return torch.tensor([[0, 0, 0, -1, 0, 0, 0, 0] + entry * capacity] * batch, dtype=torch.int32)


def _segment_rules(rules, device=None):
    rules = SegmentRules(device=device) if rules is None else rules
    if not isinstance(rules, SegmentRules):
        raise ValueError(f'rules must be a SegmentRules (got {type(rules).__name__})')
    return rules


def segment(x, output_len=None, rules=None, return_mask=False):
    """Where are the stretches of speech in these utterances?  ``x`` (B, T', C) float32 logits or log-probabilities on the device,
    ``output_len`` their valid frames (tensor, sequence or None), ``rules`` a ``SegmentRules`` (None: the defaults, 49 classes).
    Returns a ``SegmentResult`` -- with ``return_mask=True`` ``(result, mask)``, mask (B, T') uint8: 1 where the frame is speech, 0
    beyond an utterance's length.  A segment still open at an utterance's end stays open (``spans(include_open=True)``).  A fresh
    state and one step of the kernel the streams run (nbasr_ctc_segment_step): the same bits as any chunking of the frames."""
    rules = _segment_rules(rules)
    x = _logit_chunk(x, rules.classes, rules.THINGS)
    b, n, _ = x.shape
    lengths = _lengths(output_len, b, x.device)
    state = torch.empty(b, hip.ctc_segment_state_words(rules.capacity), dtype=torch.int32, device=x.device)
    mask = torch.empty(b, n, dtype=torch.uint8, device=x.device) if return_mask else None
    if b:
        hip.ctc_segment_step(x, lengths, None, state, *rules.counts, rules.speech_lo, rules.speech_hi, rules.margin, mask)
    result = SegmentResult(state)
    return (result, mask) if return_mask else result


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
        batch = _positive(batch)
        self.rules = _segment_rules(rules, device)
        super().__init__(batch, self.rules, device)

    def _fresh_rows(self):
        return _fresh_segment_state(self.batch, self.rules.capacity)

    def _step(self, x, chunk_lengths, state_out):
        r = self.rules
        hip.ctc_segment_step(x, chunk_lengths, None if self._fresh else self.state, state_out, *r.counts, r.speech_lo, r.speech_hi, r.margin)


def decode_spans(log_probs, spans, pad=0, beam_width=12, cutoff_top_n=40, *, lm=None, alpha=1.0, beta=0.0):
    """Transcribe segments: ``log_probs`` (B, T', C) float32 log-probabilities on the device, ``spans`` per row a list of ``(start,
    end, ...)`` frame spans of that tensor -- what ``SegmentResult.spans()`` returns.  Each span is widened by ``pad`` frames on both
    sides and clipped to the tensor; all spans of all rows are gathered into one padded batch by a single index operation and decoded
    by ONE ``beam_decode`` call (``beam_width``, ``cutoff_top_n``, ``lm``, ``alpha``, ``beta`` are its arguments), whose search runs one
    workgroup per utterance: each result is, to the bit, ``beam_decode`` of its slice alone.  Returns per row a list of ``(start, end,
    tokens, score)``: the span as given, the best beam's tokens (1-D int32 CPU tensor) and its score (-log P, a float).  No spans:
    empty lists, no launch."""
    if not isinstance(log_probs, torch.Tensor) or log_probs.dim() != 3:
        raise ValueError(f'log_probs must be (batch, frames, classes), got {tuple(getattr(log_probs, "shape", ()))}')
    b, t, _ = log_probs.shape
    spans = [list(row) for row in spans]
    if len(spans) != b:
        raise ValueError(f'expected the spans of {b} rows, got {len(spans)}')
    pad = int(pad)
    if pad < 0:
        raise ValueError(f'pad must not be negative (got {pad})')
    rows, first, last = [], [], []
    for i, row in enumerate(spans):
        for span in row:
            start, end = int(span[0]), int(span[1])
            if not 0 <= start <= end:
                raise ValueError(f'a span is (start, end, ...) with 0 <= start <= end (got {tuple(span)})')
            rows.append(i)
            first.append(min(max(start - pad, 0), t))
            last.append(min(end + pad, t))
    out = [[] for _ in range(b)]
    if not rows:
        return out
    lengths = torch.tensor([hi - lo for lo, hi in zip(first, last)], dtype=torch.int32)
    width = max(int(lengths.max()), 1)
    frames = (torch.tensor(first)[:, None] + torch.arange(width)[None, :]).clamp(max=max(t - 1, 0)).to(log_probs.device)
    if t:
        batch = log_probs[torch.tensor(rows, device=log_probs.device)[:, None], frames]     # (spans, width, C): frames past a span's end are not read
    else:
        batch = log_probs.new_zeros(len(rows), width, log_probs.shape[2])                   # (no frame to gather: every span is empty)
    beams, scores, out_len = beam_decode(batch, lengths, beam_width, 0, cutoff_top_n, lm=lm, alpha=alpha, beta=beta)
    beams, scores, out_len = beams[:, 0].cpu(), scores[:, 0].cpu(), out_len[:, 0].cpu()
    at = 0
    for i, row in enumerate(spans):
        for span in row:
            out[i].append((int(span[0]), int(span[1]), beams[at, :int(out_len[at])].clone(), float(scores[at])))
            at += 1
    return out


# ---- keywords: has this phrase just been said? (nbasr.h "keywords"; DESIGN.md §9 "Keywords") -------------------------------------------
MAX_KEYWORDS = 64
MAX_KEYWORD_TOKENS = hip.KEYWORD_MAX_TOKENS
_NEG_INF_BITS = -8388608         # float32 -inf as an int32


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

    OWNER, THINGS = 'the keyword spotter', 'the keywords'

    def __init__(self, keywords, thresholds=None, per_token=1.0, classes=49, blank=0, device=None):
        classes, blank = int(classes), int(blank)
        if not 2 <= classes <= MAX_ENDPOINT_CLASSES:
            raise ValueError(f'classes must lie in [2, {MAX_ENDPOINT_CLASSES}] (got {classes})')
        if not 0 <= blank < classes:
            raise ValueError(f'blank must lie in [0, {classes}) (got {blank})')
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
        from .phonemes import vocab
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

    def __repr__(self):
        return f'KeywordSet(keywords={self.keywords}, thresholds={self.thresholds}, classes={self.classes}, blank={self.blank})'


class KeywordResult:
    """The spotter's view of a batch: (B, K) device tensors, one entry per utterance and keyword.  int32 ``frames`` (frames seen),
    ``hit_frame`` / ``hit_start`` (the first frame whose score reached the threshold and the frame the path that ends there started at;
    -1: no hit yet), ``best_frame`` / ``best_start`` (the same for the highest score so far; the earliest frame on a tie), float32
    ``hit_score`` / ``best_score`` (-inf: none), and ``detected`` (bool, ``hit_frame >= 0``, computed on the device when asked for).
    Nothing here reads the device: ``bool(r.detected.any())`` is the caller's synchronisation.  The tensors are views of the state
    record they were made from: a stream's ``result`` shows its committed record and moves with the next ``push`` or ``reset()``, a
    peek's shows the peek record until the next ``peek``; ``clone()`` keeps one."""

    INT_FIELDS = {'frames': 0, 'hit_frame': 1, 'hit_start': 2, 'best_frame': 4, 'best_start': 5}
    FLOAT_FIELDS = {'hit_score': 3, 'best_score': 6}
    FIELDS = ('frames', 'hit_frame', 'hit_start', 'hit_score', 'best_frame', 'best_start', 'best_score')

    def __init__(self, state):
        self.state = state                       # (B, K, 136) int32
        as_float = state.view(torch.float32)
        for name, word in self.INT_FIELDS.items():
            setattr(self, name, state[:, :, word])
        for name, word in self.FLOAT_FIELDS.items():
            setattr(self, name, as_float[:, :, word])

    @property
    def detected(self):
        return self.hit_frame >= 0

    def clone(self):
        """A copy that no later step changes (one device copy)."""
        return KeywordResult(self.state.clone())

    def seconds(self):
        """(``hit_start``, ``hit_end``, ``best_start``, ``best_end``) as float32 device tensors of seconds from the utterance's start:
        a span runs from the START of its first frame, ``start * FRAME_SECONDS``, to the END of its last, ``(frame + 1) *
        FRAME_SECONDS``; where there is no hit (no frame yet) both are -1.0."""
        def span(first, last):
            return (torch.where(last >= 0, first.to(torch.float32) * FRAME_SECONDS, -1.0),
                    torch.where(last >= 0, (last + 1).to(torch.float32) * FRAME_SECONDS, -1.0))
        return span(self.hit_start, self.hit_frame) + span(self.best_start, self.best_frame)

    def __repr__(self):
        return 'KeywordResult(' + ', '.join(f'{name}={getattr(self, name).tolist()}' for name in self.FIELDS) + ')'


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
    if not isinstance(keywords, KeywordSet):
        raise ValueError(f'keywords must be a KeywordSet (got {type(keywords).__name__})')
    x = _logit_chunk(x, keywords.classes, keywords.THINGS)
    b, n, _ = x.shape
    k = len(keywords)
    lengths = _lengths(output_len, b, x.device)
    state = torch.empty(b, k, hip.KEYWORD_STATE_WORDS, dtype=torch.int32, device=x.device)
    scores = torch.empty(b, k, n, dtype=torch.float32, device=x.device) if return_trace else None
    starts = torch.empty(b, k, n, dtype=torch.int32, device=x.device) if return_trace else None
    if b:
        tokens, counts, thresholds = keywords.tables_on(x.device)
        hip.ctc_keyword_step(x, lengths, tokens, counts, thresholds, keywords.blank, None, state, scores, starts)
    result = KeywordResult(state)
    return (result, scores, starts) if return_trace else result


class KeywordStream(_LogitDetectorStream):
    """``spot_keywords`` fed chunk by chunk (nbasr_ctc_keyword_step with a carried state; DESIGN.md §9 "Keywords").

        kw = KeywordStream(batch, keywords, device=dev)
        r = kw.push(logits_chunk, lengths=None)  # KeywordResult of everything pushed: == spot_keywords(all frames), bit for bit
        r = kw.peek(next_chunk)                  # what push(next_chunk) would return; the stream stays as it was
        kw.result                                # the committed result; kw.reset() starts the next utterances

    The contract is ``EndpointStream``'s: both are ``_LogitDetectorStream``s, and this class adds only its record and its launch."""

    RESULT = KeywordResult

    def __init__(self, batch, keywords, device=None):
        batch = _positive(batch)
        if not isinstance(keywords, KeywordSet):
            raise ValueError(f'keywords must be a KeywordSet (got {type(keywords).__name__})')
        self.keywords = keywords
        super().__init__(batch, keywords, device)

    def _fresh_rows(self):
        return _fresh_keyword_state(self.batch, len(self.keywords))

    def _step(self, x, chunk_lengths, state_out):
        tokens, counts, thresholds = self._tables
        hip.ctc_keyword_step(x, chunk_lengths, tokens, counts, thresholds, self.keywords.blank, None if self._fresh else self.state, state_out)


# ---- confidence: how sure is the recogniser of each token? (nbasr.h "confidence"; DESIGN.md §9 "Confidence") ---------------------------
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

    OWNER, THINGS = 'the confidence estimator', 'the confidence rules'

    def __init__(self, measure='tsallis', alpha=1 / 3, blank=0, classes=49, device=None):
        if measure not in CONFIDENCE_MEASURES:
            raise ValueError(f'measure must be one of {CONFIDENCE_MEASURES} (got {measure!r})')
        if isinstance(alpha, bool) or not isinstance(alpha, (int, float)) or not 0.0 < float(alpha) < 1.0:
            raise ValueError(f'alpha must be a number strictly between 0 and 1 (got {alpha!r})')
        for name, v in (('classes', classes), ('blank', blank)):
            if isinstance(v, bool) or int(v) != v:
                raise ValueError(f'{name} must be an integer (got {v!r})')
        classes, blank = int(classes), int(blank)
        if not 2 <= classes <= MAX_ENDPOINT_CLASSES:
            raise ValueError(f'classes must lie in [2, {MAX_ENDPOINT_CLASSES}] (got {classes})')
        if not 0 <= blank < classes:
            raise ValueError(f'blank must lie in [0, {classes}) (got {blank})')
        self.measure, self.alpha, self.blank, self.classes = measure, float(alpha), blank, classes
        self.measure_index = CONFIDENCE_MEASURES.index(measure)
        self._set_device(device)

    def __repr__(self):
        return f'ConfidenceRules(measure={self.measure!r}, alpha={self.alpha}, blank={self.blank}, classes={self.classes})'


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
    rules = ConfidenceRules(device=device) if rules is None else rules
    if not isinstance(rules, ConfidenceRules):
        raise ValueError(f'rules must be a ConfidenceRules (got {type(rules).__name__})')
    return rules


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
    x = _logit_chunk(x, rules.classes, rules.THINGS)
    b, n, _ = x.shape
    lengths = _lengths(output_len, b, x.device)
    if path is not None:
        if not isinstance(path, torch.Tensor) or tuple(path.shape) != (b, n):
            raise ValueError(f'path must be a ({b}, {n}) tensor of labels, got {tuple(getattr(path, "shape", ()))}')
        path = path.to(device=x.device, dtype=torch.int32).contiguous()
    state = torch.empty(b, hip.CONFIDENCE_STATE_WORDS, dtype=torch.int32, device=x.device)
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
        batch = _positive(batch)
        self.rules = _confidence_rules(rules, device)
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
