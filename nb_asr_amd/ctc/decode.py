"""Decoding: log_softmax, greedy and prefix beam search (whole, streaming, over segments), the bigram LM and its fusion table (DESIGN.md §9 "Beam decode")."""
import torch

from . import _chunk_rows, _lengths, _positive, hip, output_lengths


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
