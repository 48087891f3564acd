"""Streaming inference: the model's forward run chunk by chunk with carried state, emitting every logit frame as soon as it is final.

    sess = model.eval().stream(batch=B, max_chunk=160)
    for chunk in chunks:                         # (B, 80, n) float32 on the model's device, any n >= 0
        logits = sess.push(chunk)                # (B, m, 49): the frames that are final now
    tail = sess.flush()                          # the rest, with the full forward's zero right-padding
    # torch.cat([*pushes, tail], 1) == model(torch.cat(chunks, 2))   (to fp32 round-off)

    logits, committed, partial = sess.push(chunk, decode='beam')       # also the prefix beam search of ctc.beam_decode
    logits, (beams, scores, out_len) = sess.flush(decode='beam')
    logits, committed, partial, committed_frames, partial_frames = sess.push(chunk, decode='beam-timed')    # + each token's output frame
    logits, (beams, scores, timesteps, out_len) = sess.flush(decode='beam-timed')

    provisional = sess.peek()                    # what flush() would return now; the session stays as it was (any time before flush)
    provisional, (beams, scores, out_len) = sess.peek(decode='beam')   # ... with flush's decode forms (True, 'beam', 'beam-timed')

    sess = model.eval().stream(batch=B, frontend=fe)                   # fe: frontend.LogMelFrontend on the model's device
    logits = sess.push_audio(wave_chunk)         # (B, n) float32 samples: the front-end's stream (frontend.FrontendStream), then push
    sess = StreamingSession(model.eval(), B, frontend=fe, input_rate=48000)      # push_audio takes samples at 48 kHz (frontend.Resampler)
    sess = StreamingSession(model.eval(), B, endpoint=ctc.EndpointRules())       # every push / flush also feeds an endpointer:
    sess.endpoint.endpoint_frame                 # (B) int32 on the device, -1 until a rule held; latched until reset()
    provisional, ahead = sess.peek_endpoint()    # peek(), and the endpointer's view with the provisional frames included
    sess = StreamingSession(model.eval(), B, keywords=ctc.KeywordSet.from_phonemes([['sh', 'iy']]))      # ... and a keyword spotter:
    sess.keywords.hit_frame                      # (B, K) int32 on the device, -1 until keyword k's score reached its threshold; latched
    provisional, ahead = sess.peek_keywords()    # peek(), and the spotter's view with the provisional frames included
    sess = StreamingSession(model.eval(), B, segments=ctc.SegmentRules())        # ... and a segmenter, which never latches:
    sess.segments.count                          # (B) int32 on the device: segments closed so far; sess.segments.spans() reads them
    provisional, ahead = sess.peek_segments()    # peek(), and the segmenter's view with the provisional frames included
    sess = StreamingSession(model.eval(), B, confidence=ctc.ConfidenceRules())   # ... and per-token confidence:
    sess.confidence.last.tokens_list()           # per row [(label, start, end, mean, min)]: the tokens the latest push / flush closed
    provisional, ahead = sess.peek_confidence()  # peek(), and the tokens that would close if the audio stopped now
    sess = StreamingSession(model.to(torch.bfloat16).eval(), B, dtype=torch.bfloat16)      # the bf16 storage path, live: bfloat16 chunks in,
    logits = sess.push(chunk.to(torch.bfloat16))                                           # bfloat16 logits out; everything above applies

Why this is exact: every convolution of the model pads at most ``context / stride`` frames on the right (reference
ops.py:8-17), LayerNorm, ``linear`` and ``zero`` have no time extent and the LSTM is unidirectional, so an output frame depends on a
bounded window of future input frames plus the LSTM state.  The model is cut into STAGES -- the four downsample convolutions with their
LayerNorms, each SearchCell, the LSTM, the head -- and every stage keeps, in a window of its own, the input frames its next outputs still
need (its left context) plus the frames that arrived since.  A push recomputes each stage over its window with the whole-forward kernels
(which zero-pad the window on both sides) and keeps exactly the outputs whose receptive field lies inside the window -- or touches the
utterance's true start / end, where the full forward's padding is the same zeros.

``StreamPlanner`` is that geometry in pure python (no HIP calls: tests/test_streaming_host.py drives the CPU oracle through it);
``StreamingSession`` executes it on the device.
"""
import torch

from . import hip
from .ctc import (BeamSearchStream, ConfidenceRules, ConfidenceStream, EndpointRules, EndpointStream, KeywordSet, KeywordStream, SegmentRules,
                  SegmentStream, empty_beam_result, fusion_table)
from .frontend import LogMelFrontend, Resampler, end_frames_bound, frames_final

FEATURES = 80
FILTERS = (600, 800, 1000, 1200)
CELLS_PER_BLOCK = (3, 4, 5, 6)
DOWN_KERNEL = 8
DOWN_STRIDES = (1, 1, 2, 2)
LSTM_HIDDEN = 500
CONTEXT = 4
OP_NAMES = ('linear', 'conv5', 'conv5d2', 'conv7', 'conv7d2', 'zero')
CONV_OPS = {'conv5': (5, 1), 'conv5d2': (5, 2), 'conv7': (7, 1), 'conv7d2': (7, 2)}
BEAM_DECODES = ('beam', 'beam-timed')               # ``decode=`` values of a session that run the prefix beam search


def pad_amounts(kernel, dilation, stride, context=CONTEXT):
    """(left, right) zero padding of a PadConvRelu: the host rule of ``nbasr_pad_amounts`` (reference ops.py:12-17), restated so that the
    planner runs without the library."""
    look_ahead = int(context / stride)
    span = kernel * dilation - stride
    if look_ahead >= span:
        return 0, span
    return int((kernel - 1) * dilation - look_ahead), look_ahead


def out_length(frames, stride):
    return (frames + stride - 1) // stride


def _names(arch):
    """arch vector ([[op index, flags...], ...]) or names ([[op name, flags...], ...]) -> names."""
    return [[OP_NAMES[n[0]] if isinstance(n[0], int) else n[0]] + [int(f) for f in n[1:]] for n in arch]


def cell_context(arch):
    """(left, right) context of a SearchCell in frames, path by path: a node's reach is the larger of its main op's padding plus the reach
    of the op's input (not for ``zero``: it reads nothing) and the reach of each flagged skip input; the cell's is its last node's."""
    reach = [(0, 0)]                                     # of the cell input, then of every node output
    for op, *flags in _names(arch):
        cands = [reach[i] for i, f in enumerate(flags) if f]
        if op != 'zero':
            lpad, rpad = (0, 0) if op == 'linear' else pad_amounts(*CONV_OPS[op], 1)
            cands.append((lpad + reach[-1][0], rpad + reach[-1][1]))
        reach.append((max(c[0] for c in cands), max(c[1] for c in cands)) if cands else (0, 0))
    return reach[-1]


class StageSpec:
    """One stage: ``kind`` in dense / cell / lstm / head, the index of its (first) layer in ``model.model``, its stride, left / right context
    in its own input frames, channels in / out, and ``rate``: model input frames per input frame of the stage."""

    def __init__(self, kind, layer, blk, stride, left, right, c_in, c_out, rate):
        self.kind, self.layer, self.blk, self.stride, self.left, self.right = kind, layer, blk, stride, left, right
        self.c_in, self.c_out, self.rate = c_in, c_out, rate

    def __repr__(self):
        return f'StageSpec({self.kind}, layer={self.layer}, stride={self.stride}, ctx=({self.left}, {self.right}), rate={self.rate})'


def stage_specs(arch, use_rnn=True, use_norm=True):
    """The stages of the model in order (``use_norm`` does not move a frame: LayerNorm works per frame)."""
    specs, idx, rate, c_in = [], 0, 1, FEATURES
    cl, cr = cell_context(arch)
    for blk, c in enumerate(FILTERS):
        s = DOWN_STRIDES[blk]
        lpad, rpad = pad_amounts(DOWN_KERNEL, 1, s)
        specs.append(StageSpec('dense', idx, blk, s, lpad, rpad, c_in, c, rate))
        idx += 2                                                          # the conv, then its block LayerNorm
        rate *= s
        for _ in range(CELLS_PER_BLOCK[blk]):
            specs.append(StageSpec('cell', idx, blk, 1, cl, cr, c, c, rate))
            idx += 1
        c_in = c
    if use_rnn:
        idx += 1                                                          # (nn.Dropout: the identity here)
        specs.append(StageSpec('lstm', idx, None, 1, 0, 0, FILTERS[-1], LSTM_HIDDEN, rate))
        idx += 1
        c_in = LSTM_HIDDEN
    specs.append(StageSpec('head', idx, None, 1, 0, 0, c_in, None, rate))
    return specs


def lookahead_frames(specs):
    """Input frames an output frame waits for beyond its own position: output o is final once input frame 4 o + lookahead has arrived."""
    return sum(s.right * s.rate for s in specs)


class StagePlan:
    """What one stage does in one step.  Absolute frames of the stage's input: the window it computes over is [a, b); it is built from
    ``n_hist`` retained frames (starting ``hist_off`` into the previous window) and ``n_new`` new ones.  It keeps the absolute output
    frames [c, d) -- positions [c - a / stride, d - a / stride) of its output over the window.  ``compute`` False: only the window moves
    (no new output yet); a stage with no plan in a step launches nothing."""

    __slots__ = ('a', 'b', 'c', 'd', 'hist_off', 'n_hist', 'n_new', 'compute')

    def __init__(self, **kw):
        for k, v in kw.items():
            setattr(self, k, v)

    @property
    def keep(self):
        return self.c, self.d

    def __repr__(self):
        return f'StagePlan(window=[{self.a}, {self.b}), keep=[{self.c}, {self.d}), hist={self.n_hist}, new={self.n_new})'


class StreamPlanner:
    """The geometry of a streaming session (pure python).  ``step(n)`` advances by n input frames (``final=True``: the utterance ends
    after them) and returns one ``StagePlan`` or None per stage; the head's [c, d) are the logit frames emitted."""

    def __init__(self, specs):
        self.specs = list(specs)
        self.lookahead = lookahead_frames(self.specs)
        self.reset()

    def reset(self):
        n = len(self.specs)
        self.have = [0] * n          # input frames received per stage
        self.done = [0] * n          # output frames emitted per stage
        self.start = [0] * n         # absolute first frame of the stage's current window
        self.next_start = [0] * n    # ... of its next one
        self.finished = False

    def step(self, n_new, final=False):
        if self.finished:
            raise ValueError('the utterance has ended (flush); reset() starts the next one')
        plans = []
        for k, sp in enumerate(self.specs):
            s = sp.stride
            if n_new == 0 and not final:
                plans.append(None)
                continue
            old_have = self.have[k]
            have = self.have[k] = old_have + n_new
            a = self.next_start[k]
            if final:
                d = out_length(have, s)
            else:
                d = max(self.done[k], (have - 1 - sp.right) // s + 1)
            c = self.done[k]
            if n_new == 0 and d == c:
                plans.append(None)                      # nothing arrives, nothing is released
                n_new = 0
                continue
            plans.append(StagePlan(a=a, b=have, c=c, d=d, hist_off=a - self.start[k], n_hist=old_have - a, n_new=n_new, compute=d > c))
            self.start[k] = a
            self.done[k] = d
            nxt = max(0, s * d - sp.left)
            if s == 2:
                nxt &= ~1                                # stride-2 windows start at even frames: outputs stay on the full forward's grid
            self.next_start[k] = min(max(nxt, a), have)
            n_new = d - c
        if final:
            self.finished = True
        return plans

    def copy(self):
        """A throw-away planner in this one's state: steps on it (an uncommitted push, then the final step) leave this one alone."""
        other = StreamPlanner.__new__(StreamPlanner)
        other.specs, other.lookahead = self.specs, self.lookahead
        other.have, other.done, other.start, other.next_start = list(self.have), list(self.done), list(self.start), list(self.next_start)
        other.finished = self.finished
        return other

    def peek(self, n_new=0):
        """The plans ``step(n_new, final=True)`` would return, with the planner left as it was."""
        return self.copy().step(n_new, final=True)

    def capacities(self, max_chunk):
        """Upper bounds of every stage's window (input frames) for pushes of at most ``max_chunk`` frames and the final flush: the frames a
        step can deliver to stage k + 1 are at most new_k / s + right / s + 2, its retained history at most left + right + s + 1."""
        caps, new = [], int(max_chunk)
        for sp in self.specs:
            caps.append(new + sp.left + sp.right + sp.stride + 4)
            new = new // sp.stride + sp.right // sp.stride + 3
        return caps

    def max_provisional_frames(self, end_frames=2):
        """The most output frames a peek can return (host only; a session sizes its beam peek workspace with it, once): the largest
        ``output_frames(f + end_frames) - done[-1]`` after f single-frame steps (f = 0 included: a peek before any frame is in),
        ``end_frames`` being a front-end's end frames (``frontend.end_frames_bound``: 2, more behind a resampler with many pending
        outputs).  The emitted count is a function of the frames received alone and repeats with period 4 once frames are emitted, so
        the first lookahead + 32 show it."""
        probe, most = StreamPlanner(self.specs), 1
        for f in range(0, self.lookahead + 33):
            if f:
                probe.step(1)
            total = f + end_frames
            for sp in self.specs:
                total = out_length(total, sp.stride)
            most = max(most, total - probe.done[-1])
        return most


def node_names(cell):
    """A SearchCell's nodes as ``stage_specs`` takes them: [[op name, identity flag per skip input...], ...]."""
    from .ops import PadConvRelu, Linear, Zero
    conv_names = {shape: name for name, shape in CONV_OPS.items()}
    names = []
    for node in cell.nodes:
        op = node.op
        if isinstance(op, PadConvRelu):
            name = conv_names[(op.kernel_size, op.dilation)]
        elif isinstance(op, Linear):
            name = 'linear'
        elif isinstance(op, Zero):
            name = 'zero'
        else:
            raise ValueError(f'unsupported node operation {type(op).__name__}')
        names.append([name] + [int(type(br).__name__ == 'Identity') for br in node.branch_ops])
    return names


class _Carried:
    """What a step reads and advances, and nothing else: the planner, per stage the current window as (buffer, row pitch), whether the
    LSTM has started with its ``h`` / ``c`` tensors (None without the LSTM), the greedy decoder's previous token, the frame counters.
    A session owns the committed one; its first ``peek`` makes a second with tensors of its own, and every peek steps on that one after
    ``refresh`` -- which is why a peek leaves the session as it was."""

    def __init__(self, planner, buffers, h, c, prev_token):
        self.planner, self.h, self.c, self.prev_token = planner, h, c, prev_token
        self.window = [(b, 0) for b in buffers]
        self.reset()

    def reset(self):
        self.planner.reset()
        self.window = [(b, 0) for b, _ in self.window]
        self.lstm_started = False
        self.frames_in = self.frames_out = 0
        self.prev_token.fill_(-1)

    def refresh(self, other):
        """Take ``other``'s state: steps on this record then leave ``other`` alone."""
        self.planner = other.planner.copy()
        self.window = list(other.window)
        self.lstm_started = other.lstm_started
        self.frames_in, self.frames_out = other.frames_in, other.frames_out
        self.prev_token.copy_(other.prev_token)
        if other.lstm_started:                   # (the recurrence's cell_ws is in/out)
            self.c.copy_(other.c)
            self.h.copy_(other.h)


# ------------------------------------------------------------------------------------------------------------------------------------
class StreamingSession:
    """Chunk-by-chunk forward of ``model`` for a lockstep batch of ``batch`` utterances (``ASRModel.stream``).  Owns its windows, LSTM
    state and packed weights (never a plan of ``model._plans``: plain ``model(x)`` calls in between keep working); every launch goes to
    the caller's current stream.  Memory depends on (batch, max_chunk, architecture) only and is allocated here.  ``lm``, ``alpha``,
    ``beta``: the bigram fusion of ``ctc.beam_decode`` for the session's beam searches (``decode='beam'`` and ``'beam-timed'``);
    ``ASRModel.stream`` keeps its parameter list, so a session with an LM is made with this constructor, which takes ``stream``'s
    arguments after the model.  ``input_rate``: the sample rate of what ``push_audio`` is given, when it is not the front-end's
    (``frontend.Resampler``: a HIP resampler ahead of the front-end's stream; DESIGN.md 9 "Resampler").  ``None`` or the front-end's own
    rate is the session without the argument, launch for launch.  ``lookahead_samples`` is then in samples at the input rate.
    ``endpoint``: a ``ctc.EndpointRules``; the session then keeps a ``ctc.EndpointStream`` and every push / push_audio / flush hands it
    the logits it returns, after the decode launches -- one more launch when the step emitted a frame, none otherwise (``endpoint``,
    ``peek_endpoint``; DESIGN.md 9 "Endpoint").  ``None`` is the session without the argument: nothing allocated, nothing launched.
    ``keywords``: a ``ctc.KeywordSet``; the session then keeps a ``ctc.KeywordStream`` and hands it the same logits after the decode
    and endpoint launches, again one more launch when the step emitted a frame (``keywords``, ``peek_keywords``; DESIGN.md 9
    "Keywords").  ``None``: nothing allocated, nothing launched.
    ``segments``: a ``ctc.SegmentRules``; the session then keeps a ``ctc.SegmentStream`` and hands it the same logits after the decode,
    endpoint and keyword launches, again one more launch when the step emitted a frame (``segments``, ``peek_segments``; DESIGN.md 9
    "Segments").  Its frames are logit frames since ``reset()``; ``flush()`` leaves an open segment open, and the caller ends it at
    ``frames``.  ``None``: nothing allocated, nothing launched.
    ``confidence``: a ``ctc.ConfidenceRules``; the session then keeps a ``ctc.ConfidenceStream`` and hands it the same logits after the
    decode launches and BEFORE the other listeners -- one more launch when the step emitted a frame; ``flush()`` hands it ``final=True``,
    which closes the token still open and is one launch even with no frame (``confidence``, ``peek_confidence``; DESIGN.md 9
    "Confidence").  ``None``: nothing allocated, nothing launched.
    ``dtype``: None (float32) or the storage type of the model's parameters; anything else, or a model stored otherwise, is refused.
    ``dtype=torch.bfloat16`` with a bfloat16 model (``model.to(torch.bfloat16)``) is the bfloat16 session (DESIGN.md 9 "bf16 sessions"):
    the windows in front of every encoder stage and the LSTM hold bfloat16 rows (pitch 8 frames, built by nbasr_stream_window_bf16), the
    stages run the bf16 matrix-core kernels with every LayerNorm where ``walk.WalkBf16`` places it, gates, h, c and the logits ahead of
    their one rounding stay float32.  ``push`` takes bfloat16 chunks, ``push_audio`` float32 samples as ever (the front-end's float32
    frames are rounded while the first window is built); ``push`` / ``flush`` / ``peek`` return bfloat16 logits, as ``model(x)`` does,
    and the decoders and listeners read ``logits.float()`` of exactly those (one more conversion per result).  A float32 session is
    launch for launch the session without the argument; a bfloat16 model without it is refused."""

    def __init__(self, model, batch, max_chunk=160, beam_width=12, cutoff_top_n=40, frontend=None, *, dtype=None, input_rate=None,
                 confidence=None, endpoint=None, keywords=None, segments=None, lm=None, alpha=1.0, beta=0.0):
        if frontend is not None and not isinstance(frontend, LogMelFrontend):
            raise ValueError(f'frontend must be a LogMelFrontend or None (got {type(frontend).__name__})')
        if confidence is not None and not isinstance(confidence, ConfidenceRules):
            raise ValueError(f'confidence must be a ctc.ConfidenceRules or None (got {type(confidence).__name__})')
        if endpoint is not None and not isinstance(endpoint, EndpointRules):
            raise ValueError(f'endpoint must be a ctc.EndpointRules or None (got {type(endpoint).__name__})')
        if keywords is not None and not isinstance(keywords, KeywordSet):
            raise ValueError(f'keywords must be a ctc.KeywordSet or None (got {type(keywords).__name__})')
        if segments is not None and not isinstance(segments, SegmentRules):
            raise ValueError(f'segments must be a ctc.SegmentRules or None (got {type(segments).__name__})')
        resampler = self.resampler_for(frontend, input_rate, getattr(frontend, 'device', None))
        self.end_frames = self.check_max_chunk(max_chunk, frontend, resampler)
        p0 = model.model[0].conv.weight
        if dtype not in (None, torch.float32, torch.bfloat16):
            raise ValueError(f'dtype must be torch.float32, torch.bfloat16 or None (float32), got {dtype!r}')
        if dtype is None and p0.dtype != torch.float32:
            raise ValueError(f'streaming runs float32 models unless asked: StreamingSession(model, batch, dtype=torch.bfloat16) streams a bfloat16 model '
                             f'(this one is {p0.dtype})')
        self.dtype = torch.float32 if dtype is None else dtype
        if p0.dtype != self.dtype:
            raise ValueError(f'dtype={self.dtype} does not match the model, whose parameters are {p0.dtype}: a session runs the model as it is stored')
        if model.training and model.dropout_rate > 0:
            raise ValueError('streaming has no dropout masks: call model.eval() or build the model with dropout_rate=0.0')
        if not p0.is_cuda:
            raise ValueError('the model must live on a HIP device (this package has no CPU path)')
        batch, max_chunk = int(batch), int(max_chunk)
        if batch < 1 or max_chunk < 1:
            raise ValueError(f'batch and max_chunk must be positive (got {batch}, {max_chunk})')
        self.model, self.batch, self.max_chunk, self.device = model, batch, max_chunk, p0.device
        self.beam_width, self.cutoff_top_n = int(beam_width), int(cutoff_top_n)
        self._lm = None if lm is None else fusion_table(lm, alpha, beta, p0.device)              # validated here; handed on as built
        self._beams = {}                          # decode value -> ctc.BeamSearchStream, made by the first push / peek that decodes so
        self._peek = None                         # the _Carried a peek steps on; with the engine's peek windows, made by the first peek
        self._peek_frames = None
        names = node_names(model.model[2])
        self.specs = stage_specs(names, model.use_rnn, model.use_norm)
        planner = StreamPlanner(self.specs)
        self.lookahead_frames = planner.lookahead
        self.caps = caps = planner.capacities(max_chunk)
        dev, B = self.device, batch
        # everything a step touches on the device: the stage engine of the storage type.  The session holds it, it never holds the
        # session, and no bound method of either is stored: a dropped session frees its memory at once (stream_stages.py)
        from .stream_stages import StagesBf16, StagesF32
        self._stages = stages = (StagesBf16 if self.dtype == torch.bfloat16 else StagesF32)(model, self.specs, caps, B, dev)
        self._carried = _Carried(planner, [bufs[0] for bufs in stages.windows], stages.h, stages.c, stages.buf(B, torch.int32)[:B])
        # from the waveform: the front-end's stream and the staging buffer its frames are written to (one model step at a time)
        self._frontend, self._resampler, self.lookahead_samples = None, None, None
        if frontend is not None:
            if frontend.device != dev:
                raise ValueError(f'the front-end lives on {frontend.device}, the model on {dev}')
            if frontend.n_mels != FEATURES:
                raise ValueError(f'the model reads {FEATURES} features per frame, the front-end makes {frontend.n_mels}')
            self._frontend = frontend.stream(B)
            ld = hip.round_up4(max_chunk)
            self._staging = stages.buf(B * FEATURES * ld).view(B, FEATURES, ld)
            self.lookahead_samples = self._frontend.lookahead_samples + frontend.hop_length * self.lookahead_frames
            if resampler is not None:            # in samples at the input rate: the front-end's share converted, plus the resampler's own
                self._resampler = resampler.stream(B)
                self.lookahead_samples = -(-self.lookahead_samples * resampler.o // resampler.n) + resampler.lookahead_samples
        self._confidence = self._listener(ConfidenceStream, confidence, 'the confidence rules')    # (steps ahead of the listeners, and knows the end)
        self._endpoint = self._listener(EndpointStream, endpoint, 'the endpoint rules')
        self._keywords = self._listener(KeywordStream, keywords, 'the keywords')
        self._segments = self._listener(SegmentStream, segments, 'the segment rules')
        # what hears the logits of every step, in launch order (after the decode launches): another detector is one more entry
        self._listeners = [d for d in (self._endpoint, self._keywords, self._segments) if d is not None]
        # everything with ``state_bytes`` (the decoders join it as they are made): what ``buffer_bytes`` adds up
        self._stateful = [d for d in (stages, self._frontend, self._resampler, self._confidence, *self._listeners) if d is not None]
        self.reset()

    def _listener(self, stream, spec, what):
        """The ``ctc`` detector stream of this session for ``spec`` (its rules or keywords; None: no such listener)."""
        if spec is None:
            return None
        classes = self.model.model[self.specs[-1].layer].out_features
        if spec.classes != classes:
            raise ValueError(f'{what} are for {spec.classes} classes, the model has {classes}')
        return stream(self.batch, spec, self.device)

    @staticmethod
    def resampler_for(frontend, input_rate, device):
        """The ``Resampler`` of a session fed samples at ``input_rate``; None when they arrive at the front-end's own rate (``None`` or
        that rate: exactly the session without the argument)."""
        if input_rate is None:
            return None
        if frontend is None:
            raise ValueError('input_rate needs a front-end: model.stream(..., frontend=LogMelFrontend(...), input_rate=...)')
        if int(input_rate) == frontend.sample_rate:
            return None
        return Resampler(input_rate, frontend.sample_rate, device=device)

    @staticmethod
    def check_max_chunk(max_chunk, frontend, resampler):
        """The most frames the front-end emits for an utterance's end (``frontend.end_frames_bound``; 2 without a resampler).  Behind a
        resampler a peek takes them in two steps ahead of the final one, as flush does -- the frames the resampler's pending outputs
        complete, then the front-end's end frames -- and has two places to build their windows, so each must be ONE step: a
        ``max_chunk`` below the bound is refused."""
        if frontend is None:
            return 2
        if resampler is None:
            return end_frames_bound(0, frontend.hop_length, frontend.n_fft)
        bound = end_frames_bound(resampler.max_pending, frontend.hop_length, frontend.n_fft)
        if int(max_chunk) < bound:
            raise ValueError(f'max_chunk={max_chunk} is below the {bound} frames that end an utterance resampled from {resampler.orig_freq} Hz '
                             f'({resampler.max_pending} outputs can be pending): a peek has no place for more steps')
        return bound

    # ---- public ----------------------------------------------------------------------------------------------------------------
    frames_in = property(lambda self: self._carried.frames_in, doc='input frames taken in this utterance')
    frames_out = property(lambda self: self._carried.frames_out, doc='logit frames returned in this utterance')
    prev_token = property(lambda self: self._carried.prev_token, doc='(batch) int32: the greedy decoder\'s last argmax, -1 at the start')

    @property
    def buffer_bytes(self):
        """Device bytes the session owns (windows, scratch, LSTM state, packed weights, the beam search state once it exists, with a
        front-end its sample tails and the staging buffer, with ``endpoint=`` the endpointer's state, with ``keywords=`` the spotter's,
        with ``segments=`` the segmenter's, with ``confidence=`` the estimator's, and from the first ``peek`` on the peek's scratch
        window, state copies and beam workspace)."""
        return sum(d.state_bytes for d in self._stateful) + sum(d.peek_bytes for d in self._beams.values())

    @property
    def endpoint(self):
        """The ``ctc.EndpointResult`` of the logit frames returned so far in this utterance (device tensors, no synchronisation); None for
        a session made without ``endpoint=``.  Once ``endpoint_frame >= 0`` it stays until ``reset()``: committed frames never change."""
        return None if self._endpoint is None else self._endpoint.result

    @property
    def keywords(self):
        """The ``ctc.KeywordResult`` of the logit frames returned so far in this utterance ((B, K) device tensors, no synchronisation);
        None for a session made without ``keywords=``.  Once ``hit_frame >= 0`` the hit stays until ``reset()``; ``best_*`` go on improving."""
        return None if self._keywords is None else self._keywords.result

    @property
    def segments(self):
        """The ``ctc.SegmentResult`` of the logit frames returned since ``reset()`` (device tensors; only its ``spans()`` reads the
        device); None for a session made without ``segments=``.  Frames are logit frames since ``reset()``.  A closed segment stays as
        it is (until the ring of ``capacity`` entries turns over it); ``flush()`` leaves an open segment open: it ends at ``frames``."""
        return None if self._segments is None else self._segments.result

    @property
    def confidence(self):
        """The session's ``ctc.ConfidenceStream``; None for a session made without ``confidence=``.  Its ``last`` is the
        ``ctc.ConfidenceResult`` of the latest push / push_audio / flush: the tokens that step closed (device tensors; only
        ``tokens_list()`` reads the device).  A token closes at the first frame that does not continue it; ``flush()`` closes the last."""
        return self._confidence

    def reset(self):
        """Start a new batch of utterances; the buffers are re-used."""
        self._carried.reset()
        self._flushed = False
        self._beam_frames = 0                    # logit frames fed to the beam search in this utterance
        self._beam_mode = None                   # 'beam' or 'beam-timed': the decoder that has seen this utterance's frames
        for mode in sorted(self._beams):         # ('beam' before 'beam-timed')
            self._beams[mode].reset()
        self._fed = None                         # 'features' (push) or 'audio' (push_audio): one utterance takes one of them
        if self._frontend is not None:
            self._frontend.reset()
        if self._resampler is not None:
            self._resampler.reset()
        if self._confidence is not None:
            self._confidence.reset()
        for d in self._listeners:
            d.reset()

    def push(self, chunk, decode=False):
        """Feed (batch, 80, n) frames of the session's dtype (float32; bfloat16 in a bfloat16 session); returns the logits (batch, m, 49)
        that became final (m >= 0) -- with ``decode=True`` also the greedy CTC tokens of those frames (a list of int32 CPU tensors),
        repeats collapsed across pushes.  ``decode='beam'`` returns
        ``(logits, committed, partial)``: the prefix beam search of ``ctc.beam_decode`` run over the log-probabilities of the final frames
        (``ctc.BeamSearchStream``): tokens that are now final, and the best beam's tokens after all committed ones.
        ``decode='beam-timed'`` returns ``(logits, committed, partial, committed_frames, partial_frames)``: the same search with each
        token's time step (``BeamSearchStream(timesteps=True)``), an output-frame index -- one output frame is 4 input frames, 40 ms at
        the front-end's 10 ms hop.  One utterance is decoded with one of the two."""
        if self._flushed:
            raise ValueError('push after flush: call reset() to start the next utterance')
        if not isinstance(chunk, torch.Tensor) or chunk.dim() != 3 or chunk.shape[0] != self.batch or chunk.shape[1] != FEATURES:
            raise ValueError(f'expected a ({self.batch}, {FEATURES}, frames) chunk, got {tuple(getattr(chunk, "shape", ()))}')
        if not self._stages.accepts(chunk):
            raise ValueError(f'the chunk must be {self._stages.name} on {self.device} (got {chunk.dtype} on {chunk.device})')
        if self._fed == 'audio':
            raise ValueError('push after push_audio: an utterance is fed features or samples, not both (reset() starts the next one)')
        self._begin(decode)
        self._fed = 'features'
        chunk = chunk.detach().contiguous()
        outs = [self._commit(chunk, off, n) for off, n in self._cuts(chunk.shape[2])] or [self._commit(None, 0, 0)]
        return self._result(outs, decode)

    def push_audio(self, wave_chunk, decode=False):
        """Feed (batch, n) float32 samples of the waveform (a session made with ``frontend=``): the front-end's stream turns them into the
        frames that are final now (``frontend.FrontendStream``, one launch per ``max_chunk`` frames, written to the session's staging
        buffer), and those go the way of ``push`` -- same steps, same results, same ``decode`` forms as pushing them as features."""
        if self._frontend is None:
            raise ValueError('push_audio needs a front-end: model.stream(..., frontend=LogMelFrontend(...))')
        if self._flushed:
            raise ValueError('push after flush: call reset() to start the next utterance')
        if self._fed == 'features':
            raise ValueError('push_audio after push: an utterance is fed features or samples, not both (reset() starts the next one)')
        if (not isinstance(wave_chunk, torch.Tensor) or wave_chunk.dim() != 2 or wave_chunk.shape[0] != self.batch
                or (wave_chunk.dtype, wave_chunk.device) != (torch.float32, self.device)):
            raise ValueError(f'expected a ({self.batch}, samples) float32 chunk on {self.device}, got {tuple(getattr(wave_chunk, "shape", ()))} '
                             f'{getattr(wave_chunk, "dtype", None)} on {getattr(wave_chunk, "device", None)}')
        self._begin(decode)
        self._fed = 'audio'
        if self._resampler is not None:          # samples at the input rate: the outputs that are final now go on as the push
            wave_chunk = self._resampler.push(wave_chunk)
        outs = [self._commit(self._staging if k else None, 0, k) for k in self._frontend.push_tiled(wave_chunk, self._staging, self.max_chunk)]
        return self._result(outs, decode)

    def flush(self, decode=False):
        """End the utterance: the remaining logits, computed with the full forward's zero right-padding.  ``decode='beam'`` returns
        ``(logits, (beams, scores, out_len))``: ``ctc.beam_decode`` of the log-probabilities of all the utterance's logits;
        ``decode='beam-timed'`` ``(logits, (beams, scores, timesteps, out_len))``, its ``return_timesteps=True`` form."""
        if self._flushed:
            raise ValueError('flush called twice: call reset() to start the next utterance')
        self._begin(decode)
        outs = []
        if self._fed == 'audio':                 # the front-end's last 1 or 2 frames first, as a push of features
            if self._resampler is not None:      # (ahead of them the resampler's last outputs, as a push of samples)
                ahead = self._frontend.samples_in + self._resampler.pending
                if ahead <= self._frontend.win // 2:         # refused as the front-end's flush refuses it, before anything moves
                    raise ValueError(f'reflect padding needs more than {self._frontend.win // 2} samples (the utterance has {ahead} at '
                                     f'{self._frontend.frontend.sample_rate} Hz)')
                last = self._resampler.flush()
                outs = [self._commit(self._staging if k else None, 0, k) for k in self._frontend.push_tiled(last, self._staging, self.max_chunk)]
            m = self._frontend.flush(out=(self._staging, 0)).shape[2]
            outs += [self._commit(self._staging, off, n) for off, n in self._cuts(m)]
        outs.append(self._commit(None, 0, 0, final=True))
        self._flushed = True
        return self._result(outs, decode, final=True)

    def peek(self, decode=False):
        """What ``flush(decode)`` would return now, without ending anything: the provisional logits (batch, m, 49) of the output frames
        [frames_out, output_frames(frames_in)) -- with a front-end, ``frames_in`` after its end frames -- computed with the utterance-end
        zero padding in place of the right context that has not arrived.  ``decode`` as ``flush``: ``True`` -> ``(logits, tokens)``,
        ``'beam'`` -> ``(logits, (beams, scores, out_len))``, ``'beam-timed'`` -> ``(logits, (beams, scores, timesteps, out_len))`` over
        all the utterance's frames so far.  The session is left exactly as it was (DESIGN.md 9 "Peek"): every later push / flush / peek
        returns the bits it would have returned without this call.  Before any frame: (batch, 0, 49) and empty hypotheses, no launch
        (behind a resampler: unless its pending outputs would carry the front-end past ``win // 2`` samples, as they would at a flush)."""
        if self._flushed:
            raise ValueError('peek after flush: call reset() to start the next utterance')
        self._stages.check_params()
        if decode in BEAM_DECODES:
            self._beam_check(decode)
        resampled = self._resampler is not None and self._fed == 'audio'
        # behind a resampler its pending outputs come with the end: they can carry the front-end past win // 2 before any frame is in
        endable = resampled and self._frontend.samples_in + self._resampler.pending > self._frontend.win // 2
        if self.frames_in == 0 and not endable:  # (with a front-end: at most win // 2 samples so far, too few to end an utterance)
            logits = self._stages.logits(0)
            if decode in BEAM_DECODES:
                return logits, empty_beam_result(self.batch, self.beam_width, self.device, decode == 'beam-timed')
            return (logits, [torch.zeros(0, dtype=torch.int32) for _ in range(self.batch)]) if decode else logits
        pk, stages = self._peek_record(), self._stages
        outs = []
        places = (stages.place_other, stages.place_third)
        if resampled:                            # flush's steps: the frames the resampler's last outputs complete, then the end frames
            fs, extra = self._frontend, self._resampler.peek()
            m = fs.peek(out=(self._staging, 0), extra=extra).shape[2]
            first = frames_final(fs.samples_in + extra.shape[1], fs.hop, fs.win) - fs.frames_out
            cuts = [(off, n) for off, n in ((0, first), (first, m - first)) if n]          # (each at most end_frames <= max_chunk)
            outs = [stages.step(pk, self._staging, off, n, False, places[i]) for i, (off, n) in enumerate(cuts)]
        elif self._fed == 'audio':               # the front-end's end frames as uncommitted pushes, then the final step
            m = self._frontend.peek(out=(self._staging, 0)).shape[2]
            outs = [stages.step(pk, self._staging, off, n, False, places[i]) for i, (off, n) in enumerate(self._cuts(m))]
        outs.append(stages.step(pk, None, 0, 0, True, stages.place_peek))
        logits = stages.join(outs)
        if decode in BEAM_DECODES:
            dec = self._decoder(decode)
            dec.reserve_peek(self._peek_frames, logits.shape[2])
            return logits, dec.peek(self._log_probs(stages.heard(logits)))
        return (logits, self._greedy(pk, stages.heard(logits))) if decode else logits

    def peek_endpoint(self, decode=False):
        """``(peek(decode), EndpointResult)``: one peek of the model, then the endpointer's peek over the provisional logits on top of its
        committed state -- ``ctc.endpoint`` of the committed and the provisional frames together.  A peeked endpoint is PROVISIONAL:
        the provisional frames are computed as if the audio stopped now and can change when more arrives, so an endpoint seen here
        can disappear; a committed one (``endpoint``) cannot.  The session and its endpointer are left as they were."""
        return self._peek_with(self._endpoint, 'peek_endpoint needs endpoint rules: StreamingSession(..., endpoint=ctc.EndpointRules(...))', decode)

    def peek_keywords(self, decode=False):
        """``(peek(decode), KeywordResult)``: one peek of the model, then the spotter's peek over the provisional logits on top of its
        committed state -- ``ctc.spot_keywords`` of the committed and the provisional frames together.  A peeked hit is PROVISIONAL:
        the provisional frames are computed as if the audio stopped now and can change when more arrives, so a hit seen here can
        disappear; a committed one (``keywords``) cannot.  The session and its spotter are left as they were."""
        return self._peek_with(self._keywords, 'peek_keywords needs a keyword set: StreamingSession(..., keywords=ctc.KeywordSet(...))', decode)

    def peek_segments(self, decode=False):
        """``(peek(decode), SegmentResult)``: one peek of the model, then the segmenter's peek over the provisional logits on top of its
        committed state -- ``ctc.segment`` of the committed and the provisional frames together.  A peeked segment is PROVISIONAL:
        the provisional frames are computed as if the audio stopped now and can change when more arrives, so a segment seen opening
        or closing here can do so elsewhere, or not at all; the committed ones (``segments``) cannot.  The session and its segmenter
        are left as they were."""
        return self._peek_with(self._segments, 'peek_segments needs segment rules: StreamingSession(..., segments=ctc.SegmentRules(...))', decode)

    def peek_confidence(self, decode=False):
        """``(peek(decode), ConfidenceResult)``: one peek of the model, then the estimator's final peek over the provisional logits on top
        of its committed state -- the tokens that would close if the audio stopped now, the open one included.  What it shows is
        PROVISIONAL: the provisional frames are computed as if the audio stopped now and can change when more arrives, so a token
        seen here can end elsewhere, with another confidence, or not be there at all; the tokens of ``confidence.last`` cannot.  The
        session and its estimator are left as they were."""
        return self._peek_with(self._confidence, 'peek_confidence needs confidence rules: StreamingSession(..., confidence=ctc.ConfidenceRules(...))',
                               decode)

    def _peek_with(self, listener, refusal, decode):
        """``(peek(decode), the listener's peek over the provisional logits)``; ``refusal``: what a session without that listener says."""
        if listener is None:
            raise ValueError(refusal)
        peeked = self.peek(decode)
        logits = peeked if isinstance(peeked, torch.Tensor) else peeked[0]
        return peeked, listener.peek(self._stages.heard(logits))

    def _peek_record(self):
        """The record a peek steps on, in the committed one's present state.  The first peek allocates it, with the windows only a peek
        builds: the scratch window (sized for the largest stage window) and, for a session that pushes the front-end's two end frames
        in two steps (``max_chunk`` 1), a third buffer per stage."""
        if self._peek is None:
            thirds = self._frontend is not None and (self.max_chunk < 2 or self._resampler is not None)
            self._peek_frames = self._carried.planner.max_provisional_frames(self.end_frames)      # the beam peek workspace is sized once, for these
            self._peek = _Carried(self._carried.planner.copy(), [], *self._stages.peek_state(self._carried, thirds))
        self._peek.refresh(self._carried)
        return self._peek

    def _beam_check(self, decode):
        if self._beam_mode not in (None, decode):
            raise ValueError(f"decode={decode!r} after decode={self._beam_mode!r} in one utterance: one search sees every frame "
                             '(call reset() to start the next utterance with the other)')
        if self._beam_frames != self.frames_out:
            raise ValueError(f"decode={decode!r} must see every logit frame of the utterance: use it from the first push on (or reset())")

    def _begin(self, decode):
        """Before a push or flush moves a frame: refuse stale weights, and what its beam search could not do."""
        self._stages.check_params()
        if decode in BEAM_DECODES:
            self._beam_check(decode)
            self._beam_mode = decode
            self._decoder(decode)

    def _decoder(self, decode):
        if decode not in self._beams:
            self._beams[decode] = BeamSearchStream(self.batch, self.beam_width, 0, self.cutoff_top_n, self.device,
                                                   timesteps=decode == 'beam-timed', lm=self._lm)
            self._stateful.append(self._beams[decode])
        return self._beams[decode]

    @staticmethod
    def _log_probs(logits):
        return hip.ctc_postprocess(logits, None, True, False)[0] if logits.shape[1] else logits

    def _greedy(self, rec, logits):
        """The greedy tokens of ``logits``, repeats collapsed against (and carried on in) ``rec.prev_token``."""
        tokens, counts = hip.ctc_greedy_stream(logits, rec.prev_token)
        tokens, counts = tokens.cpu(), counts.cpu()
        return [tokens[i, : int(counts[i])] for i in range(self.batch)]

    def _result(self, outs, decode, final=False):
        """What push / push_audio / flush return for their steps' logits."""
        logits, heard = self._stages.join(outs), self._stages.heard
        if decode in BEAM_DECODES:
            dec = self._decoder(decode)
            self._beam_frames += logits.shape[1]
            pushed = dec.push(self._log_probs(heard(logits)))
            result = (logits, dec.finish()) if final else (logits,) + pushed
        else:
            result = (logits, self._greedy(self._carried, heard(logits))) if decode else logits
        if self._confidence is not None:         # after the decode launches, ahead of the listeners; the only one that is told the end
            self._confidence.push(heard(logits), final=final)
        for d in self._listeners:                # endpoint, keywords, segments; a step that emitted no frame launches nothing
            d.push(heard(logits))
        return result

    def _cuts(self, n):
        """(first frame, frames) of the steps that take n frames."""
        return [(off, min(self.max_chunk, n - off)) for off in range(0, n, self.max_chunk)]

    def _commit(self, chunk, off, n, final=False):
        """A committed step: the session's own record, every stage's window built in its pair's other buffer."""
        return self._stages.step(self._carried, chunk, off, n, final, self._stages.place_other)
