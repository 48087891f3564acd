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


class _Bf16Copies:
    """What ``executor.node_into(..., copies=)`` reads of a bfloat16 session's derived weights: the four lookups of a ``ForwardPlan`` it
    uses, answered from what the session packed once (``kept``: fp32 copies by ``id(parameter)``; ``packed``: the session's images)."""

    def __init__(self, kept, packed, pointwise_ws):
        self.kept, self.packed, self.pointwise_ws = kept, packed, pointwise_ws

    def _f32(self, param):
        return self.kept[id(param)]

    def _packed_grouped(self, op):
        return self.packed[id(op)]

    def _packed_linear_bf16(self, w):
        return self.packed[id(w)]

    def _pointwise_bf16_ws(self, batch, c_in, ld):
        return self.pointwise_ws


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
        self._peek = None                         # the _Carried a peek steps on; with its windows below, made by the first peek
        self._peek_window = self._peek_thirds = self._peek_frames = None
        names = node_names(model.model[2])
        self.specs = stage_specs(names, model.use_rnn, model.use_norm)
        planner = StreamPlanner(self.specs)
        self.lookahead_frames = planner.lookahead
        self.caps = caps = planner.capacities(max_chunk)
        dev, B = self.device, batch
        self._bufs = []

        def buf(numel, dtype=torch.float32):
            t = torch.empty(max(int(numel), 4), device=dev, dtype=dtype)
            self._bufs.append(t)
            return t

        if self.dtype == torch.bfloat16:
            h, c = self._allocate16(names, buf)
        else:
            h, c = self._allocate(names, buf)
        self._carried = _Carried(planner, [bufs[0] for bufs in self.windows], h, c, buf(B, torch.int32)[:B])
        # per stage kind (its body and what builds its window, None: no window -- the functions: bound methods would make the session hold itself)
        cls = StreamingSession
        if self.dtype == torch.bfloat16:
            bodies = {'dense': (cls._dense16, cls._window16), 'cell': (cls._cell16, cls._window16), 'lstm': (cls._lstm16, cls._window16),
                      'head': (cls._head_of_lstm16, None) if model.use_rnn else (cls._head16, cls._window)}
        else:
            bodies = {'dense': (cls._dense, cls._window), 'cell': (cls._cell, cls._window), 'lstm': (cls._lstm, cls._window),
                      'head': (cls._head_of_lstm, None) if model.use_rnn else (cls._head, cls._window)}
        self._bodies = [bodies[sp.kind] for sp in self.specs]
        # from the waveform: the front-end's stream and the staging buffer its frames are written to (one model step at a time)
        self._frontend, self._resampler, self.lookahead_samples = None, None, None
        if frontend is not None:
            if frontend.device != dev:
                raise ValueError(f'the front-end lives on {frontend.device}, the model on {dev}')
            if frontend.n_mels != FEATURES:
                raise ValueError(f'the model reads {FEATURES} features per frame, the front-end makes {frontend.n_mels}')
            self._frontend = frontend.stream(B)
            ld = hip.round_up4(max_chunk)
            self._staging = buf(B * FEATURES * ld).view(B, FEATURES, ld)
            self.lookahead_samples = self._frontend.lookahead_samples + frontend.hop_length * self.lookahead_frames
            if resampler is not None:            # in samples at the input rate: the front-end's share converted, plus the resampler's own
                self._resampler = resampler.stream(B)
                self.lookahead_samples = -(-self.lookahead_samples * resampler.o // resampler.n) + resampler.lookahead_samples
        self._pack16() if self.dtype == torch.bfloat16 else self._pack()
        self._confidence = self._listener(ConfidenceStream, confidence, 'the confidence rules')    # (steps ahead of the listeners, and knows the end)
        self._endpoint = self._listener(EndpointStream, endpoint, 'the endpoint rules')
        self._keywords = self._listener(KeywordStream, keywords, 'the keywords')
        self._segments = self._listener(SegmentStream, segments, 'the segment rules')
        # what hears the logits of every step, in launch order (after the decode launches): another detector is one more entry
        self._listeners = [d for d in (self._endpoint, self._keywords, self._segments) if d is not None]
        self.reset()

    def _allocate(self, names, buf):
        """The float32 session's windows and scratch (``buf``: the constructor's allocator); returns the LSTM's (h, c) or (None, None)."""
        model, caps, B = self.model, self.caps, self.batch
        # a pair of windows per stage (the head / LSTM input: one buffer, nothing is retained), scratch for outputs and node results
        self.windows = []
        out_elems = node_elems = need_pw = 0
        has_linear = any(n[0] == 'linear' for n in names)
        for sp, cap in zip(self.specs, caps):
            ld = hip.round_up4(cap)
            n = B * sp.c_in * ld
            self.windows.append([buf(n), buf(n)] if sp.kind in ('dense', 'cell') else [buf(n)])
            if sp.kind in ('dense', 'cell'):
                out_elems = max(out_elems, B * sp.c_out * hip.round_up4(out_length(cap, sp.stride)))
            if sp.kind == 'cell':
                node_elems = max(node_elems, B * sp.c_out * ld)
            if sp.kind == 'lstm' or (sp.kind == 'cell' and has_linear):
                need_pw = max(need_pw, hip.load_library().nbasr_pointwise_workspace_bytes(B, sp.c_in, ld))
        self.scratch = buf(out_elems)
        self.node_scratch = [buf(node_elems), buf(node_elems)]
        self.absmax = buf(B)[:B]
        self.pointwise_ws = buf(need_pw, torch.uint8) if need_pw else None
        h = c = None
        if model.use_rnn:
            lstm_cap = caps[[sp.kind for sp in self.specs].index('lstm')]
            self.gates = buf(lstm_cap * B * 4 * LSTM_HIDDEN)
            self.h_out = buf(B * lstm_cap * LSTM_HIDDEN)
            h, c = buf(B * LSTM_HIDDEN), buf(B * LSTM_HIDDEN)
            self.xcd_ws = buf(hip.lstm_xcd_workspace_bytes(B, LSTM_HIDDEN), torch.uint8)
        return h, c

    def _allocate16(self, names, buf):
        """The bfloat16 session's windows and scratch: bf16 rows pitched to 8 frames in front of every encoder stage and the LSTM (fp32
        rows in front of a head without LSTM: the last LayerNorm writes fp32), bf16 scratch; LayerNorm statistics, gates, h, c and the
        logits ahead of their rounding in fp32.  Fixes what must not depend on a push's frame count: whether the cells run on the
        matrix cores (they do where the stage's largest window fits; else every window takes the node launches)."""
        from .walk import _CELL_SKIPS
        from .ops import PadConvRelu, Identity
        model, caps, B, lib = self.model, self.caps, self.batch, hip.load_library()
        bf16 = torch.bfloat16
        cells = [(sp, hip.round_up8(cap)) for sp, cap in zip(self.specs, caps) if sp.kind == 'cell']
        nodes = model.model[cells[0][0].layer].nodes
        conv_only = len(nodes) == 3 and all(isinstance(n.op, PadConvRelu) and n.op.groups > 1 for n in nodes)
        self._cell_mfma = conv_only and all(hip.grouped_cell_mfma_fits(sp.c_in, ld, model.model[sp.layer].nodes[-1].op.groups) for sp, ld in cells)
        self._skip_mask = sum(1 << bit for bit, (j, i) in enumerate(_CELL_SKIPS) if isinstance(nodes[j].branch_ops[i], Identity)) if conv_only else 0
        self.windows = []
        out_elems = node_elems = need_pw = image_bytes = 0
        has_linear = any(n[0] == 'linear' for n in names)
        for sp, cap in zip(self.specs, caps):
            ld = hip.round_up8(cap)
            n = B * sp.c_in * ld
            if sp.kind == 'head':                # behind the LSTM: no window; without it: fp32 rows
                self.windows.append([buf(0 if model.use_rnn else B * sp.c_in * hip.round_up4(cap))])
                continue
            self.windows.append([buf(n, bf16), buf(n, bf16)] if sp.kind in ('dense', 'cell') else [buf(n, bf16)])
            if sp.kind in ('dense', 'cell'):
                out_elems = max(out_elems, B * sp.c_out * hip.round_up8(out_length(cap, sp.stride)))
            if sp.kind == 'dense':
                image_bytes = max(image_bytes, lib.nbasr_bf16_image_bytes(B, sp.c_in, ld))
            if sp.kind == 'cell' and not self._cell_mfma:
                node_elems = max(node_elems, B * sp.c_out * ld)
            if sp.kind == 'lstm' or (sp.kind == 'cell' and has_linear):
                need_pw = max(need_pw, lib.nbasr_pointwise_bf16_workspace_bytes(B, sp.c_in, ld))
        ld_max = hip.round_up8(max(caps))
        self.scratch = buf(out_elems, bf16)
        self.node_scratch = [buf(node_elems, bf16), buf(node_elems, bf16)] if node_elems else None
        self.stats = buf(B * 2 * ld_max)         # per-frame (mean, rstd) of the LayerNorm a stage applies while it loads its window
        self.image = buf(max(image_bytes, 16), torch.uint8)
        self.pointwise_ws = buf(max(need_pw, 16), torch.uint8) if need_pw else None
        classes = model.model[self.specs[-1].layer].out_features
        self.logits32 = buf(hip.round_up8(B * max(caps[-2:]) * classes))
        h = c = None
        if model.use_rnn:
            lstm_cap = caps[[sp.kind for sp in self.specs].index('lstm')]
            self.gates = buf(lstm_cap * B * 4 * LSTM_HIDDEN)
            self.h_out = buf(B * lstm_cap * LSTM_HIDDEN)
            h, c = buf(B * LSTM_HIDDEN), buf(B * LSTM_HIDDEN)
            self.xcd_ws = buf(hip.lstm_xcd_workspace_bytes(B, LSTM_HIDDEN), torch.uint8)
        else:
            sp, ld = cells[-1]
            self.enc32 = buf(B * sp.c_out * ld)  # the encoder output as the head reads it
        return h, c

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

    # ---- weights ---------------------------------------------------------------------------------------------------------------
    def _pack(self):
        """Derived weight copies, made once; ``push`` refuses to run once a parameter has changed (its version counter moved)."""
        import torch.nn as nn
        from .ops import PadConvRelu, Linear
        m = self.model.model
        self._versions = [(p, p.data_ptr(), p._version) for p in self.model.parameters()]
        self._packed = {}
        with torch.no_grad():
            for sp in self.specs:
                if sp.kind == 'dense':
                    conv = m[sp.layer]
                    scheme = 'bf16x3' if sp.blk == 0 else 'f16x2'
                    self._packed[sp.layer] = (scheme, hip.pack_dense_weights(conv.conv.weight.detach(), conv.strides, scheme))
                elif sp.kind == 'cell':
                    for node in m[sp.layer].nodes:
                        if isinstance(node.op, PadConvRelu):
                            self._packed[id(node.op)] = hip.pack_grouped_weights(node.op.conv.weight.detach().contiguous(), node.op.groups)
                        elif isinstance(node.op, Linear):
                            self._packed[id(node.op.linear)] = hip.pack_pointwise_weights(node.op.linear.weight.detach())
                elif sp.kind == 'lstm':
                    lstm = m[sp.layer]
                    assert isinstance(lstm, nn.LSTM)
                    self._packed['w_ih'] = hip.pack_pointwise_weights(lstm.weight_ih_l0.detach())
                    self._packed['w_hh16'] = hip.lstm_pack_whh16(lstm.weight_hh_l0.detach().contiguous())
        self._bufs.extend(t for t in self._packed.values() if isinstance(t, torch.Tensor))
        self._bufs.extend(t for _, t in (v for v in self._packed.values() if isinstance(v, tuple)))

    def _pack16(self):
        """The bfloat16 session's derived weights, made once: the operand images the matrix-core kernels take (packed from fp32 copies
        that are dropped again) and fp32 copies of what the kernels read as fp32 -- biases, gamma / beta, the head.  Also settles, per
        stage, where its LayerNorm is applied (``walk.WalkBf16``'s placement): ``_ln_in[k]`` = (gamma, beta, eps) of the LayerNorm stage k
        applies while it loads its un-normalised window, ``_ln_out[k]`` = (how, gamma, beta, eps) of the one it applies to its output
        ('inplace': bf16 rows for a cell that starts with `linear`; 'f32': fp32 rows for the head, gamma None: only widened)."""
        import torch.nn as nn
        from . import tiles
        from .ops import PadConvRelu, Linear
        from .walk import cheap_consumer
        m, B = self.model.model, self.batch
        self._versions = [(p, p.data_ptr(), p._version) for p in self.model.parameters()]
        self._packed, kept = {}, {}

        def f32(p):
            return p.detach().float().contiguous()

        def keep(p):
            if id(p) not in kept:
                kept[id(p)] = f32(p)
            return kept[id(p)]

        norms = [None] * len(self.specs)         # the LayerNorm behind each stage
        with torch.no_grad():
            for k, (sp, cap) in enumerate(zip(self.specs, self.caps)):
                if sp.kind == 'dense':
                    conv, norms[k] = m[sp.layer], m[sp.layer + 1]
                    # the row tile of the stage's largest window, for every push: one packed image (every tiling gives the same bits)
                    rows, ftile = tiles.bf16_tile(B, sp.c_out, out_length(cap, sp.stride))
                    self._packed[sp.layer] = (hip.pack_dense_weights_bf16(f32(conv.conv.weight), conv.strides, rows), rows, ftile)
                    keep(conv.conv.bias)
                elif sp.kind == 'cell':
                    cell = m[sp.layer]
                    norms[k] = cell.norm_layer if cell.use_norm else None
                    for node in cell.nodes:
                        op = node.op
                        if isinstance(op, PadConvRelu):
                            w = f32(op.conv.weight)
                            self._packed[id(op)] = hip.grouped_cell_mfma_pack(w, op.groups) if self._cell_mfma else hip.pack_grouped_weights(w, op.groups)
                            keep(op.conv.bias)
                        elif isinstance(op, Linear):
                            self._packed[id(op.linear.weight)] = hip.pack_pointwise_weights_bf16(f32(op.linear.weight))
                            keep(op.linear.bias)
                elif sp.kind == 'lstm':
                    lstm = m[sp.layer]
                    assert isinstance(lstm, nn.LSTM)
                    self._packed['w_ih'] = hip.pack_pointwise_weights_bf16(f32(lstm.weight_ih_l0))
                    self._packed['w_hh16'] = hip.lstm_pack_whh16(f32(lstm.weight_hh_l0))
                    keep(lstm.bias_ih_l0), keep(lstm.bias_hh_l0)
                else:
                    keep(m[sp.layer].weight), keep(m[sp.layer].bias)
            self._ln_in, self._ln_out = [None] * len(self.specs), [None] * len(self.specs)
            for k, norm in enumerate(norms):
                if self.specs[k].kind not in ('dense', 'cell'):
                    continue
                nxt = self.specs[k + 1]
                affine = (None, None, 0.0) if norm is None else (keep(norm.weight), keep(norm.bias), norm.eps)
                if nxt.kind == 'head':
                    self._ln_out[k] = ('f32',) + affine
                elif norm is not None and nxt.kind == 'cell' and not cheap_consumer(m[nxt.layer]):
                    self._ln_out[k] = ('inplace',) + affine
                elif norm is not None:           # a conv-only cell, a dense conv's operand image, the LSTM's projection: on load
                    self._ln_in[k + 1] = affine
        self._copies = _Bf16Copies(kept, self._packed, self.pointwise_ws)
        self._bufs.extend(kept.values())
        self._bufs.extend(v[0] if isinstance(v, tuple) else v for v in self._packed.values())

    def _check_params(self):
        for p, ptr, ver in self._versions:
            if p.data_ptr() != ptr or p._version != ver:
                raise ValueError('a parameter of the model changed after the session packed its weights: create a new session')
        if len(self._versions) != len(list(self.model.parameters())):
            raise ValueError('the model\'s parameters changed after the session packed its weights: create a new session')

    # ---- public ----------------------------------------------------------------------------------------------------------------
    frames_in = property(lambda self: self._carried.frames_in, doc='input frames taken in this utterance')
    frames_out = property(lambda self: self._carried.frames_out, doc='logit frames returned in this utterance')
    prev_token = property(lambda self: self._carried.prev_token, doc='(batch) int32: the greedy decoder\'s last argmax, -1 at the start')

    @property
    def buffer_bytes(self):
        """Device bytes the session owns (windows, scratch, LSTM state, packed weights, the beam search state once it exists, with a
        front-end its sample tails and the staging buffer, with ``endpoint=`` the endpointer's state, with ``keywords=`` the spotter's, with ``segments=``
        the segmenter's, with ``confidence=`` the estimator's, and from the first ``peek`` on the peek's scratch window, state copies and beam workspace)."""
        return (sum(t.numel() * t.element_size() for t in self._bufs)
                + sum(d.state_bytes + d.peek_bytes for d in self._beams.values())
                + (self._frontend.state_bytes if self._frontend is not None else 0)
                + (self._resampler.state_bytes if self._resampler is not None else 0)
                + sum(d.state_bytes for d in self._listeners) + (self._confidence.state_bytes if self._confidence is not None else 0))

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
        """Feed (batch, 80, n) frames of the session's dtype (float32; bfloat16 in a bfloat16 session); returns the logits (batch, m, 49) that became final (m >= 0) -- with ``decode=True`` also
        the greedy CTC tokens of those frames (a list of int32 CPU tensors), repeats collapsed across pushes.  ``decode='beam'`` returns
        ``(logits, committed, partial)``: the prefix beam search of ``ctc.beam_decode`` run over the log-probabilities of the final frames
        (``ctc.BeamSearchStream``): tokens that are now final, and the best beam's tokens after all committed ones.
        ``decode='beam-timed'`` returns ``(logits, committed, partial, committed_frames, partial_frames)``: the same search with each
        token's time step (``BeamSearchStream(timesteps=True)``), an output-frame index -- one output frame is 4 input frames, 40 ms at
        the front-end's 10 ms hop.  One utterance is decoded with one of the two."""
        if self._flushed:
            raise ValueError('push after flush: call reset() to start the next utterance')
        if not isinstance(chunk, torch.Tensor) or chunk.dim() != 3 or chunk.shape[0] != self.batch or chunk.shape[1] != FEATURES:
            raise ValueError(f'expected a ({self.batch}, {FEATURES}, frames) chunk, got {tuple(getattr(chunk, "shape", ()))}')
        if chunk.dtype != self.dtype or chunk.device != self.device:
            name = 'bfloat16' if self.dtype == torch.bfloat16 else 'float32'
            raise ValueError(f'the chunk must be {name} on {self.device} (got {chunk.dtype} on {chunk.device})')
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
                or wave_chunk.dtype != torch.float32 or wave_chunk.device != self.device):
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
        self._check_params()
        if decode in BEAM_DECODES:
            self._beam_check(decode)
        resampled = self._resampler is not None and self._fed == 'audio'
        # behind a resampler its pending outputs come with the end: they can carry the front-end past win // 2 before any frame is in
        endable = resampled and self._frontend.samples_in + self._resampler.pending > self._frontend.win // 2
        if self.frames_in == 0 and not endable:  # (with a front-end: at most win // 2 samples so far, too few to end an utterance)
            logits = self._logits(0)
            if decode in BEAM_DECODES:
                return logits, empty_beam_result(self.batch, self.beam_width, self.device, decode == 'beam-timed')
            return (logits, [torch.zeros(0, dtype=torch.int32) for _ in range(self.batch)]) if decode else logits
        pk = self._peek_record()
        outs = []
        places = (self._place_other, lambda k, current: self._peek_thirds[k])
        if resampled:                            # flush's steps: the frames the resampler's last outputs complete, then the end frames
            fs, extra = self._frontend, self._resampler.peek()
            m = fs.peek(out=(self._staging, 0), extra=extra).shape[2]
            first = frames_final(fs.samples_in + extra.shape[1], fs.hop, fs.win) - fs.frames_out
            cuts = [(off, n) for off, n in ((0, first), (first, m - first)) if n]          # (each at most end_frames <= max_chunk)
            outs = [self._step(pk, self._staging, off, n, False, places[i]) for i, (off, n) in enumerate(cuts)]
        elif self._fed == 'audio':               # the front-end's end frames as uncommitted pushes, then the final step
            m = self._frontend.peek(out=(self._staging, 0)).shape[2]
            outs = [self._step(pk, self._staging, off, n, False, places[i]) for i, (off, n) in enumerate(self._cuts(m))]
        outs.append(self._step(pk, None, 0, 0, True, self._place_peek))
        logits = self._join(outs)
        if decode in BEAM_DECODES:
            dec = self._decoder(decode)
            dec.reserve_peek(self._peek_frames, logits.shape[2])
            return logits, dec.peek(self._log_probs(self._heard(logits)))
        return (logits, self._greedy(pk, self._heard(logits))) if decode else logits

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
        return peeked, listener.peek(self._heard(logits))

    def _peek_record(self):
        """The record a peek steps on, in the committed one's present state.  The first peek allocates it, with the windows only a peek
        builds: the scratch window (sized for the largest stage window) and, for a session that pushes the front-end's two end frames
        in two steps (``max_chunk`` 1), a third buffer per stage."""
        if self._peek is None:
            if self._frontend is not None and (self.max_chunk < 2 or self._resampler is not None):
                self._peek_thirds = [torch.empty_like(bufs[0]) for bufs in self.windows]
                self._bufs.extend(self._peek_thirds)
            nbytes = max(bufs[0].numel() * bufs[0].element_size() for bufs in self.windows)
            self._peek_window = torch.empty(-(-nbytes // 4), device=self.device, dtype=torch.float32)
            h, c = (None if t is None else torch.empty_like(t) for t in (self._carried.h, self._carried.c))
            prev_token = torch.empty(max(self.batch, 4), device=self.device, dtype=torch.int32)
            self._bufs.extend(t for t in (self._peek_window, h, c, prev_token) if t is not None)
            self._peek_frames = self._carried.planner.max_provisional_frames(self.end_frames)      # the beam peek workspace is sized once, for these
            self._peek = _Carried(self._carried.planner.copy(), [], h, c, prev_token[:self.batch])
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
        self._check_params()
        if decode in BEAM_DECODES:
            self._beam_check(decode)
            self._beam_mode = decode
            self._decoder(decode)

    def _decoder(self, decode):
        if decode not in self._beams:
            self._beams[decode] = BeamSearchStream(self.batch, self.beam_width, 0, self.cutoff_top_n, self.device,
                                                   timesteps=decode == 'beam-timed', lm=self._lm)
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
        logits = self._join(outs)
        if decode in BEAM_DECODES:
            dec = self._decoder(decode)
            self._beam_frames += logits.shape[1]
            pushed = dec.push(self._log_probs(self._heard(logits)))
            result = (logits, dec.finish()) if final else (logits,) + pushed
        else:
            result = (logits, self._greedy(self._carried, self._heard(logits))) if decode else logits
        if self._confidence is not None:         # after the decode launches, ahead of the listeners; the only one that is told the end
            self._confidence.push(self._heard(logits), final=final)
        for d in self._listeners:                # endpoint, keywords, segments; a step that emitted no frame launches nothing
            d.push(self._heard(logits))
        return result

    def _join(self, outs):
        """The logits of several steps as one tensor.  bfloat16: over a buffer padded to 8 elements (``nbasr_flat``), as a step's are."""
        if len(outs) == 1:
            return outs[0]
        if self.dtype != torch.bfloat16:
            return torch.cat(outs, 1)
        frames = sum(o.shape[1] for o in outs)
        if frames == 0:
            return outs[0]
        logits = self._rounded(frames)
        torch.cat(outs, 1, out=logits)
        return logits

    def _rounded(self, frames):
        """(batch, frames, classes) bfloat16 logits over a buffer of whole 8-element chunks (``nbasr_flat``): what nbasr_convert works in."""
        shape = (self.batch, frames, self.model.model[self.specs[-1].layer].out_features)
        n = shape[0] * shape[1] * shape[2]
        flat = torch.empty(max(hip.round_up8(n), 8), device=self.device, dtype=torch.bfloat16)
        logits = flat[:n].view(shape)
        logits.nbasr_flat = flat
        return logits

    def _heard(self, logits):
        """What the decoders and listeners read: the logits themselves; of a bfloat16 session their fp32 widening (one nbasr_convert,
        made once per result), so that every decode result is the offline function's on ``logits.float()``."""
        if logits.dtype == torch.float32:
            return logits
        wide = getattr(logits, 'nbasr_wide', None)
        if wide is None:
            if logits.shape[1] == 0:
                wide = torch.empty(logits.shape, device=self.device, dtype=torch.float32)
            else:
                flat = logits.nbasr_flat
                wide = hip.convert(flat, torch.empty(flat.shape, device=self.device, dtype=torch.float32))[:logits.numel()].view(logits.shape)
            logits.nbasr_wide = wide
        return wide

    # ---- one step ----------------------------------------------------------------------------------------------------------------
    # Where a step builds stage k's new window is all that tells a committed step from the steps of a peek: ``place(k, current)``,
    # ``current`` the buffer that holds the stage's window now.  A committed step and a peek's first push: the pair's other buffer
    # (``_place_other``).  A peek's second push (``max_chunk`` 1 with a front-end), whose window the final step still reads: the stage's
    # third buffer.  A peek's final step, whose windows are consumed by their own stage at once and never retained: the scratch window.
    def _place_other(self, k, current):
        bufs = self.windows[k]                   # (a one-buffer stage retains nothing: it rebuilds in place)
        return bufs[0] if current is bufs[-1] else bufs[-1]

    def _cuts(self, n):
        """(first frame, frames) of the steps that take n frames."""
        return [(off, min(self.max_chunk, n - off)) for off in range(0, n, self.max_chunk)]

    def _logits(self, frames):
        return torch.empty(self.batch, frames, self.model.model[self.specs[-1].layer].out_features, device=self.device, dtype=self.dtype)

    def _place_peek(self, k, current):
        """A peek's final step: every window in the one scratch window, seen as the stage's storage type."""
        return self._peek_window if current.dtype == torch.float32 else self._peek_window.view(current.dtype)

    def _commit(self, chunk, off, n, final=False):
        return self._step(self._carried, chunk, off, n, final, self._place_other)

    def _window(self, rec, k, plan, src, place):
        """Build stage k's window [a, b) from the retained frames of its current one and the new frames at ``src`` = (tensor, first
        column), in the buffer ``place`` names; returns (the window view, its frames)."""
        sp = self.specs[k]
        hist, dst, n_w = self._window_views(rec, k, plan, place, hip.round_up4)
        absmax = self.absmax if (sp.kind == 'dense' and sp.blk > 0) else None
        hip.stream_window(hist, plan.hist_off, plan.n_hist, src[0], src[1], plan.n_new, dst, absmax)
        return dst, n_w

    def _window16(self, rec, k, plan, src, place):
        """``_window`` for bfloat16 rows (pitch: 8 frames; no range bound).  ``src`` is bfloat16, or the front-end's float32 frames at stage 0."""
        hist, dst, n_w = self._window_views(rec, k, plan, place, hip.round_up8)
        hip.stream_window_bf16(hist, plan.hist_off, plan.n_hist, src[0], src[1], plan.n_new, dst)
        return dst, n_w

    def _window_views(self, rec, k, plan, place, pitch):
        """(the retained window or None, the new window in the buffer ``place`` names, its frames) of stage k; ``rec`` moves to the new one."""
        sp, B = self.specs[k], self.batch
        n_w = plan.b - plan.a
        if n_w > self.caps[k]:
            raise RuntimeError(f'stage {k}: window of {n_w} frames exceeds its capacity {self.caps[k]} (planner bound)')
        if len(self.windows[k]) == 1 and plan.n_hist:
            raise RuntimeError(f'stage {k} ({sp.kind}) has no context but retains {plan.n_hist} frames')
        ld = pitch(n_w)
        old, ld_old = rec.window[k]
        new = place(k, old)
        rec.window[k] = (new, ld)
        dst = new[: B * sp.c_in * ld].view(B, sp.c_in, ld)
        hist = old[: B * sp.c_in * ld_old].view(B, sp.c_in, ld_old) if plan.n_hist else None
        return hist, dst, n_w

    def _step(self, rec, chunk, off, n, final, place):
        """One step of ``rec``'s planner on the device, ``rec`` advanced by it, every new window built where ``place`` says; returns the
        step's logits."""
        plans = rec.planner.step(n, final)
        rec.frames_in += n
        out = (chunk, off)                       # (tensor, first column) of the frames the next stage appends to its window
        for k, (sp, plan, (body, windower)) in enumerate(zip(self.specs, plans, self._bodies)):
            if plan is None:                     # nothing arrives, nothing is released (a later stage may still release at flush)
                out = (None, 0)
                continue
            window = windower(self, rec, k, plan, out, place) if windower is not None else out
            out = body(self, rec, k, sp, plan, window) if plan.compute else (None, 0)      # (not: only the window moves)
        logits = out if isinstance(out, torch.Tensor) else self._logits(0)
        rec.frames_out += logits.shape[1]
        return logits

    # the stage bodies: (record, stage index, spec, plan, (window view, its frames)) -> (tensor, first column) of the outputs kept, or the logits
    def _dense(self, rec, k, sp, plan, window):
        win, n_w = window
        m, B = self.model.model, self.batch
        conv, norm = m[sp.layer], m[sp.layer + 1]
        t_out = out_length(n_w, sp.stride)
        ld = hip.round_up4(t_out)
        out = self.scratch[: B * sp.c_out * ld].view(B, sp.c_out, ld)
        scheme, packed = self._packed[sp.layer]
        hip.dense_conv1d_fused_packed(win, n_w, packed, sp.c_out, conv.kernel_size, conv.conv.bias.detach(), (), out, conv.strides,
                                      None, scheme, self.absmax if scheme == 'f16x2' else None)
        hip.layernorm_channels(out, norm.weight.detach(), norm.bias.detach(), out, t_out, norm.eps)
        return out, plan.c - plan.a // sp.stride

    def _cell(self, rec, k, sp, plan, window):
        from .executor import node_into
        from .walk import fused_cell
        win, n_w = window
        cell, B = self.model.model[sp.layer], self.batch
        ld = win.shape[2]
        out = self.scratch[: B * sp.c_out * ld].view(B, sp.c_out, ld)
        nodes = cell.nodes
        groups = getattr(nodes[-1].op, 'groups', 0)
        fused, mask = fused_cell(cell, ld)
        if fused:                                # the executor's one-launch cell (bit-identical to the three node launches)
            specs = [(self._packed[id(nd.op)], nd.op.conv.bias.detach(), nd.op.kernel_size, nd.op.dilation) for nd in nodes]
            hip.grouped_cell_fused(win, specs, mask, out, n_w, groups)
        else:
            lin_ctx = (lambda lin: self._packed[id(lin)], lambda c_in, ld_: self.pointwise_ws)
            outs = [win]
            for j, node in enumerate(nodes):
                dst = out if j == len(nodes) - 1 else self.node_scratch[j % 2][: B * sp.c_out * ld].view(B, sp.c_out, ld)
                outs.append(node_into(node, outs, n_w, dst, None, None, lin_ctx, 0))
        if cell.use_norm:
            norm = cell.norm_layer
            hip.layernorm_channels(out, norm.weight.detach(), norm.bias.detach(), out, n_w, norm.eps)
        return out, plan.c - plan.a

    def _lstm(self, rec, k, sp, plan, window):
        win, nf = window                         # no context: the window holds exactly the new frames
        lstm, B = self.model.model[sp.layer], self.batch
        gates = self.gates[: nf * B * 4 * LSTM_HIDDEN]
        hip.lstm_input_projection_packed(win, nf, self._packed['w_ih'], lstm.bias_ih_l0.detach(), lstm.bias_hh_l0.detach(), gates,
                                         LSTM_HIDDEN, self.pointwise_ws)
        return self._recur(rec, gates, nf)

    def _recur(self, rec, gates, nf):
        """The recurrence over ``nf`` frames of gates from the carried (h, c), which it advances; returns (h rows, 0)."""
        B = self.batch
        h = self.h_out[: B * nf * LSTM_HIDDEN].view(B, nf, LSTM_HIDDEN)
        h_state, c_state, cont = rec.h[: B * LSTM_HIDDEN], rec.c[: B * LSTM_HIDDEN], rec.lstm_started
        hip.lstm_recurrence_frames16_state(gates, self._packed['w_hh16'], c_state, h, self.xcd_ws,
                                           h_state if cont else None, hip.LSTM_CONTINUE if cont else 0)
        rec.lstm_started = True
        # h_n = the last frame's h becomes the next call's h0 (h_out seen as one row of nf * H floats per utterance)
        hip.stream_window(None, 0, 0, h.view(B, 1, nf * LSTM_HIDDEN), (nf - 1) * LSTM_HIDDEN, LSTM_HIDDEN, h_state.view(B, 1, LSTM_HIDDEN))
        return h, 0

    def _head_of_lstm(self, rec, k, sp, plan, source):
        head, h = self.model.model[sp.layer], source[0]              # the LSTM's (batch, frames, hidden) rows, no window
        return hip.linear_head(h, head.weight.detach(), head.bias.detach(), self._logits(h.shape[1]))

    def _head(self, rec, k, sp, plan, window):
        win, n_w = window                        # without the LSTM: reads the encoder output's pitched rows
        head = self.model.model[sp.layer]
        return hip.linear_head_bct(win, n_w, head.weight.detach(), head.bias.detach(), self._logits(n_w))

    # the bfloat16 session's bodies: bf16 rows, every LayerNorm where walk.WalkBf16 places it (_pack16)
    def _pending(self, k, win, n_w):
        """(stats, gamma, beta) of the LayerNorm stage k applies while it loads ``win``, its per-frame statistics taken here (one read
        pass; per frame, so the chunking does not reach them), and its eps; (None, 0.0) where the window holds normalised rows."""
        if self._ln_in[k] is None:
            return None, 0.0
        gamma, beta, eps = self._ln_in[k]
        B, _, ld = win.shape
        stats = self.stats[: B * 2 * ld].view(B, 2, ld)
        return (stats, gamma, beta), eps

    def _norm_out(self, k, out, frames):
        """Stage k's own LayerNorm, where it is not left to the consumer's load: in place, or as the fp32 rows the head reads."""
        if self._ln_out[k] is None:
            return out
        how, gamma, beta, eps = self._ln_out[k]
        if how == 'inplace':
            return hip.layernorm_channels(out, gamma, beta, out, frames, eps)
        enc = self.enc32[: out.numel()].view(out.shape)
        return hip.convert(out, enc) if gamma is None else hip.layernorm_channels(out, gamma, beta, enc, frames, eps)

    def _dense16(self, rec, k, sp, plan, window):
        win, n_w = window
        conv, B = self.model.model[sp.layer], self.batch
        t_out = out_length(n_w, sp.stride)
        ld = hip.round_up8(t_out)
        out = self.scratch[: B * sp.c_out * ld].view(B, sp.c_out, ld)
        ln, eps = self._pending(k, win, n_w)     # (the image pass fills the statistics itself)
        image = hip.bf16_image(win, self.image, n_w, ln and ln[1:], ln and ln[0], eps)
        packed, rows, ftile = self._packed[sp.layer]
        hip.dense_conv1d_bf16_img(image, B, sp.c_in, n_w, win.shape[2], packed, sp.c_out, conv.kernel_size, self._copies._f32(conv.conv.bias), out,
                                  conv.strides, rows, ftile)
        return self._norm_out(k, out, t_out), plan.c - plan.a // sp.stride

    def _cell16(self, rec, k, sp, plan, window):
        from .executor import node_into
        win, n_w = window
        cell, B = self.model.model[sp.layer], self.batch
        ld = win.shape[2]
        out = self.scratch[: B * sp.c_out * ld].view(B, sp.c_out, ld)
        ln0, eps = self._pending(k, win, n_w)
        if ln0 is not None:
            hip.channel_stats(win, ln0[0], n_w, eps)
        nodes = cell.nodes
        if self._cell_mfma:
            specs = [(self._packed[id(nd.op)], self._copies._f32(nd.op.conv.bias), nd.op.kernel_size, nd.op.dilation) for nd in nodes]
            hip.grouped_cell_mfma(win, specs, self._skip_mask, out, n_w, nodes[-1].op.groups, ln0)
        else:                                    # one variant for every window: GC_FPL8 is the whole forward's choice for long rows
            outs = [win]
            for j, node in enumerate(nodes):
                dst = out if j == len(nodes) - 1 else self.node_scratch[j % 2][: B * sp.c_out * ld].view(B, sp.c_out, ld)
                outs.append(node_into(node, outs, n_w, dst, ln0, None, None, hip.GC_WPERM, self._copies))
        return self._norm_out(k, out, n_w), plan.c - plan.a

    def _lstm16(self, rec, k, sp, plan, window):
        win, nf = window                         # un-normalised bf16 rows: the projection applies the last cell's LayerNorm on load
        lstm, B, f32 = self.model.model[sp.layer], self.batch, self._copies._f32
        ln, eps = self._pending(k, win, nf)
        if ln is not None:
            hip.channel_stats(win, ln[0], nf, eps)
        gates = self.gates[: nf * B * 4 * LSTM_HIDDEN]
        hip.lstm_input_projection_bf16(win, nf, self._packed['w_ih'], f32(lstm.bias_ih_l0), f32(lstm.bias_hh_l0), gates, LSTM_HIDDEN,
                                       self.pointwise_ws, ln)
        return self._recur(rec, gates, nf)

    def _round_logits(self, frames, head_into):
        """The head's fp32 logits (``head_into(out)`` writes them) rounded once to bfloat16, in whole 8-element chunks as ``WalkBf16.head``
        does: the last chunk's padding is converted too and never returned."""
        logits = self._rounded(frames)
        n8 = logits.nbasr_flat.numel()
        head_into(self.logits32[: logits.numel()].view(logits.shape))
        hip.convert(self.logits32[:n8], logits.nbasr_flat)
        return logits

    def _head_of_lstm16(self, rec, k, sp, plan, source):
        head, h, f32 = self.model.model[sp.layer], source[0], self._copies._f32
        return self._round_logits(h.shape[1], lambda out: hip.linear_head(h, f32(head.weight), f32(head.bias), out))

    def _head16(self, rec, k, sp, plan, window):
        win, n_w = window                        # fp32 rows: the last LayerNorm's, or the widened encoder output
        head, f32 = self.model.model[sp.layer], self._copies._f32
        return self._round_logits(n_w, lambda out: hip.linear_head_bct(win, n_w, f32(head.weight), f32(head.bias), out))
