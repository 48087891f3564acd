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


class _Peek:
    """What ``StreamingSession.peek`` runs on instead of the session's carried state: a planner copy, a table of every stage's current
    window (buffer, row pitch), copies of the LSTM state and of the greedy decoder's previous token.  A ping-pong pair can host ONE
    uncommitted step (built in the other buffer, the pair not flipped).  A peek of an audio session is two: the front-end's end frames
    as a push, then the final step, which would overwrite the window the push just built.  The final step's windows are consumed by
    their own stage at once and never retained, so it builds all of them in one shared scratch window (sized for the largest stage
    window).  Only a session with ``max_chunk`` 1 pushes its two end frames in two steps; it gets a third buffer per stage."""

    def __init__(self):
        self.planner = self.window = self.pushes = self.scratch_window = self.thirds = self.prev_token = self.c_state = self.h_state = None
        self._lstm_started, self.max_frames = False, 1

    def destination(self, k, other):
        """Where the step under way builds stage k's window: the final step in the scratch window, push 0 in the pair's other buffer,
        push 1 (retained for the final step, so one per stage) in a third buffer."""
        if self.pushes is None:
            return self.scratch_window
        return other if self.pushes == 0 else self.thirds[k]


# ------------------------------------------------------------------------------------------------------------------------------------
class StreamingSession:
    """Chunk-by-chunk forward of ``model`` for a lockstep batch of ``batch`` utterances (``ASRModel.stream``).  Owns its windows, LSTM
    state and packed weights (never a plan of ``model._plans``: plain ``model(x)`` calls in between keep working); every launch goes to
    the caller's current stream.  Memory depends on (batch, max_chunk, architecture) only and is allocated here.  ``lm``, ``alpha``,
    ``beta``: the bigram fusion of ``ctc.beam_decode`` for the session's beam searches (``decode='beam'`` and ``'beam-timed'``); ``ASRModel.stream`` keeps its parameter list, so a session with an LM is made with this
    constructor, which takes ``stream``'s arguments after the model."""

    def __init__(self, model, batch, max_chunk=160, beam_width=12, cutoff_top_n=40, frontend=None, *, lm=None, alpha=1.0, beta=0.0):
        from .ops import PadConvRelu, Linear, Zero
        from .frontend import LogMelFrontend
        if frontend is not None and not isinstance(frontend, LogMelFrontend):
            raise ValueError(f'frontend must be a LogMelFrontend or None (got {type(frontend).__name__})')
        p0 = model.model[0].conv.weight
        if p0.dtype != torch.float32:
            raise ValueError(f'streaming runs float32 models only (this one is {p0.dtype})')
        if model.training and model.dropout_rate > 0:
            raise ValueError('streaming has no dropout masks: call model.eval() or build the model with dropout_rate=0.0')
        if not p0.is_cuda:
            raise ValueError('the model must live on a HIP device (this package has no CPU path)')
        batch, max_chunk = int(batch), int(max_chunk)
        if batch < 1 or max_chunk < 1:
            raise ValueError(f'batch and max_chunk must be positive (got {batch}, {max_chunk})')
        self.model, self.batch, self.max_chunk, self.device = model, batch, max_chunk, p0.device
        self.beam_width, self.cutoff_top_n = int(beam_width), int(cutoff_top_n)
        from .ctc import fusion_table
        self._lm = {} if lm is None else {'lm': fusion_table(lm, alpha, beta, p0.device)}         # validated here; handed on as built
        self._beam = None                         # ctc.BeamSearchStream, made by the first push with decode='beam'
        self._beam_timed = None                   # ... with timesteps=True, by the first push with decode='beam-timed'
        self._peek = None                         # _Peek: scratch window and state copies, made by the first peek
        arch = [[type(n.op).__name__, *(int(type(br).__name__ == 'Identity') for br in n.branch_ops)] for n in model.model[2].nodes]
        names = []
        for (kind, *flags), node in zip(arch, model.model[2].nodes):
            op = node.op
            if isinstance(op, PadConvRelu):
                name = {(5, 1): 'conv5', (5, 2): 'conv5d2', (7, 1): 'conv7', (7, 2): 'conv7d2'}[(op.kernel_size, op.dilation)]
            elif isinstance(op, Linear):
                name = 'linear'
            elif isinstance(op, Zero):
                name = 'zero'
            else:
                raise ValueError(f'unsupported node operation {kind}')
            names.append([name] + flags)
        self.specs = stage_specs(names, model.use_rnn, model.use_norm)
        self.planner = StreamPlanner(self.specs)
        self.lookahead_frames = self.planner.lookahead
        caps = self.planner.capacities(max_chunk)
        self.caps = caps
        dev, B = self.device, batch
        self._bufs = []

        def buf(numel, dtype=torch.float32):
            t = torch.empty(max(int(numel), 4), device=dev, dtype=dtype)
            self._bufs.append(t)
            return t

        # ping-pong windows per stage (the head / LSTM input: one buffer, nothing is retained), scratch for outputs and node results
        self.windows, self.turn = [], [0] * len(self.specs)
        out_elems, node_elems = 0, 0
        for sp, cap in zip(self.specs, caps):
            n = B * sp.c_in * hip.round_up4(cap)
            self.windows.append([buf(n), buf(n)] if sp.kind in ('dense', 'cell') else [buf(n)])
            if sp.kind in ('dense', 'cell'):
                out_elems = max(out_elems, B * sp.c_out * hip.round_up4(out_length(cap, sp.stride)))
            if sp.kind == 'cell':
                node_elems = max(node_elems, B * sp.c_out * hip.round_up4(cap))
        self.scratch = buf(out_elems)
        self.node_scratch = [buf(node_elems), buf(node_elems)]
        self.absmax = buf(B)[:B]
        self.pointwise_ws = None
        need_pw = 0
        for sp, cap in zip(self.specs, caps):
            if sp.kind == 'lstm' or (sp.kind == 'cell' and any(n[0] == 'linear' for n in names)):
                need_pw = max(need_pw, hip.load_library().nbasr_pointwise_workspace_bytes(B, sp.c_in, hip.round_up4(cap)))
        if need_pw:
            self.pointwise_ws = buf(need_pw, torch.uint8)
        if model.use_rnn:
            lstm_cap = caps[[sp.kind for sp in self.specs].index('lstm')]
            self.gates = buf(lstm_cap * B * 4 * LSTM_HIDDEN)
            self.h_out = buf(B * lstm_cap * LSTM_HIDDEN)
            self.h_state = buf(B * LSTM_HIDDEN)
            self.c_state = buf(B * LSTM_HIDDEN)
            self.xcd_ws = buf(hip.lstm_xcd_workspace_bytes(B, LSTM_HIDDEN), torch.uint8)
        self.prev_token = buf(B, torch.int32)[:B]
        # from the waveform: the front-end's stream and the staging buffer its frames are written to (one model step at a time)
        self._frontend, self.lookahead_samples = None, None
        if frontend is not None:
            if frontend.device != dev:
                raise ValueError(f'the front-end lives on {frontend.device}, the model on {dev}')
            if frontend.n_mels != FEATURES:
                raise ValueError(f'the model reads {FEATURES} features per frame, the front-end makes {frontend.n_mels}')
            self._frontend = frontend.stream(B)
            ld = hip.round_up4(max_chunk)
            self._staging = buf(B * FEATURES * ld).view(B, FEATURES, ld)
            self.lookahead_samples = self._frontend.lookahead_samples + frontend.hop_length * self.lookahead_frames
        self._pack()
        self.reset()

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

    def _check_params(self):
        for p, ptr, ver in self._versions:
            if p.data_ptr() != ptr or p._version != ver:
                raise ValueError('a parameter of the model changed after the session packed its weights: create a new session')
        if len(self._versions) != len(list(self.model.parameters())):
            raise ValueError('the model\'s parameters changed after the session packed its weights: create a new session')

    # ---- public ----------------------------------------------------------------------------------------------------------------
    @property
    def buffer_bytes(self):
        """Device bytes the session owns (windows, scratch, LSTM state, packed weights, the beam search state once it exists, with a
        front-end its sample tails and the staging buffer, and from the first ``peek`` on the peek's scratch window, state copies and
        beam workspace)."""
        return (sum(t.numel() * t.element_size() for t in self._bufs)
                + sum(d.state_bytes + d.peek_bytes for d in (self._beam, self._beam_timed) if d is not None)
                + (self._frontend.state_bytes if self._frontend is not None else 0))

    def reset(self):
        """Start a new batch of utterances; the buffers are re-used."""
        self.planner.reset()
        self.frames_in = 0
        self.frames_out = 0
        self._flushed = False
        self._lstm_started = False
        self._ld_prev = [0] * len(self.specs)     # row pitch of every stage's current window
        self.prev_token.fill_(-1)
        self._beam_frames = 0                    # logit frames fed to the beam search in this utterance
        self._beam_mode = None                   # 'beam' or 'beam-timed': the decoder that has seen this utterance's frames
        for dec in (self._beam, self._beam_timed):
            if dec is not None:
                dec.reset()
        self._fed = None                         # 'features' (push) or 'audio' (push_audio): one utterance takes one of them
        if self._frontend is not None:
            self._frontend.reset()

    def push(self, chunk, decode=False):
        """Feed (batch, 80, n) float32 frames; returns the logits (batch, m, 49) that became final (m >= 0) -- with ``decode=True`` also
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
        if chunk.dtype != torch.float32 or chunk.device != self.device:
            raise ValueError(f'the chunk must be float32 on {self.device} (got {chunk.dtype} on {chunk.device})')
        if self._fed == 'audio':
            raise ValueError('push after push_audio: an utterance is fed features or samples, not both (reset() starts the next one)')
        self._check_params()
        if decode in BEAM_DECODES:
            self._beam_ready(decode)
        self._fed = 'features'
        chunk = chunk.detach().contiguous()
        outs, n = [], chunk.shape[2]
        for off in range(0, n, self.max_chunk):
            outs.append(self._step(chunk, off, min(self.max_chunk, n - off), False))
        if not outs:
            outs.append(self._step(None, 0, 0, False))
        return self._pushed(outs, decode)

    def _pushed(self, outs, decode):
        logits = outs[0] if len(outs) == 1 else torch.cat(outs, 1)
        if decode in BEAM_DECODES:
            return (logits,) + self._beam_push(logits, decode)
        return (logits, self._decode(logits)) if decode else logits

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
        self._check_params()
        if decode in BEAM_DECODES:
            self._beam_ready(decode)
        self._fed = 'audio'
        outs = [self._step(self._staging if k else None, 0, k, False)
                for k in self._frontend.push_tiled(wave_chunk, self._staging, self.max_chunk)]
        return self._pushed(outs, decode)

    def flush(self, decode=False):
        """End the utterance: the remaining logits, computed with the full forward's zero right-padding.  ``decode='beam'`` returns
        ``(logits, (beams, scores, out_len))``: ``ctc.beam_decode`` of the log-probabilities of all the utterance's logits;
        ``decode='beam-timed'`` ``(logits, (beams, scores, timesteps, out_len))``, its ``return_timesteps=True`` form."""
        if self._flushed:
            raise ValueError('flush called twice: call reset() to start the next utterance')
        self._check_params()
        if decode in BEAM_DECODES:
            self._beam_ready(decode)
        last = []
        if self._fed == 'audio':                 # the front-end's last 1 or 2 frames first, as a push of features
            m = self._frontend.flush(out=(self._staging, 0)).shape[2]
            last = [self._step(self._staging, off, min(self.max_chunk, m - off), False) for off in range(0, m, self.max_chunk)]
        logits = self._step(None, 0, 0, True)
        if last:
            logits = torch.cat(last + [logits], 1)
        self._flushed = True
        if decode in BEAM_DECODES:
            self._beam_push(logits, decode)
            return logits, self._beam_decoder(decode).finish()
        return (logits, self._decode(logits)) if decode else logits

    def peek(self, decode=False):
        """What ``flush(decode)`` would return now, without ending anything: the provisional logits (batch, m, 49) of the output frames
        [frames_out, output_frames(frames_in)) -- with a front-end, ``frames_in`` after its end frames -- computed with the utterance-end
        zero padding in place of the right context that has not arrived.  ``decode`` as ``flush``: ``True`` -> ``(logits, tokens)``,
        ``'beam'`` -> ``(logits, (beams, scores, out_len))``, ``'beam-timed'`` -> ``(logits, (beams, scores, timesteps, out_len))`` over
        all the utterance's frames so far.  The session is left exactly as it was (DESIGN.md 9 "Peek"): every later push / flush / peek
        returns the bits it would have returned without this call.  Before any frame: (batch, 0, 49) and empty hypotheses, no launch."""
        if self._flushed:
            raise ValueError('peek after flush: call reset() to start the next utterance')
        self._check_params()
        if decode in BEAM_DECODES:
            self._beam_check(decode)
        B, classes = self.batch, self.model.model[self.specs[-1].layer].out_features
        if self.frames_in == 0:                  # (with a front-end: at most win // 2 samples so far, too few to end an utterance)
            logits = torch.empty(B, 0, classes, device=self.device, dtype=torch.float32)
            if decode in BEAM_DECODES:           # the empty prefix alone, at -log P = -0.0: finish() of a search that saw no frame
                W = self.beam_width
                scores = torch.full((B, W), torch.finfo(torch.float32).max)
                scores[:, 0] = -0.0
                none, lens = torch.zeros(B, W, 0, dtype=torch.int32).to(self.device), torch.zeros(B, W, dtype=torch.int32).to(self.device)
                return logits, ((none, scores.to(self.device), none.clone(), lens) if decode == 'beam-timed' else (none, scores.to(self.device), lens))
            return (logits, [torch.zeros(0, dtype=torch.int32) for _ in range(B)]) if decode else logits
        pk = self._peek_begin()
        outs = []
        if self._fed == 'audio':                 # the front-end's end frames as an uncommitted push, then the final step
            m = self._frontend.peek(out=(self._staging, 0)).shape[2]
            for off in range(0, m, self.max_chunk):
                outs.append(self._step(self._staging, off, min(self.max_chunk, m - off), False, pk))
                pk.pushes += 1
        pk.pushes = None
        outs.append(self._step(None, 0, 0, True, pk))
        logits = outs[0] if len(outs) == 1 else torch.cat(outs, 1)
        if decode in BEAM_DECODES:
            self._beam_make(decode)
            dec = self._beam_decoder(decode)
            dec.reserve_peek(pk.max_frames, classes)
            return logits, dec.peek(hip.ctc_postprocess(logits, None, True, False)[0] if logits.shape[1] else logits)
        if decode:
            pk.prev_token.copy_(self.prev_token)
            tokens, counts = hip.ctc_greedy_stream(logits, pk.prev_token)
            tokens, counts = tokens.cpu(), counts.cpu()
            return logits, [tokens[i, : int(counts[i])] for i in range(B)]
        return logits

    def _peek_begin(self):
        """The peek context (``_Peek``), armed with the session's present state; its buffers are allocated by the first peek."""
        if self._peek is None:
            B, pk = self.batch, _Peek()
            n = max(B * sp.c_in * hip.round_up4(cap) for sp, cap in zip(self.specs, self.caps))
            numels = [n]
            if self._frontend is not None and self.max_chunk < 2:
                pk.thirds = [torch.empty_like(bufs[0]) for bufs in self.windows]
                self._bufs.extend(pk.thirds)
            if self.model.use_rnn:
                numels += [B * LSTM_HIDDEN] * 2
            bufs = [torch.empty(max(k, 4), device=self.device, dtype=torch.float32) for k in numels] + [torch.empty(max(B, 4), device=self.device, dtype=torch.int32)]
            self._bufs.extend(bufs)
            pk.prev_token = bufs.pop()[:B]
            if self.model.use_rnn:
                pk.c_state, pk.h_state = bufs.pop(), bufs.pop()
            pk.scratch_window = bufs.pop()
            # the most output frames a peek can return (its beam workspace is sized once): the emitted count is a function of frames_in alone
            # and repeats with period 4 once frames are emitted, so the first lookahead + 32 input frames (+ 2 front-end end frames) show it
            probe, pk.max_frames = StreamPlanner(self.specs), 1
            for f in range(1, self.lookahead_frames + 33):
                probe.step(1)
                total = f + 2
                for sp in self.specs:
                    total = out_length(total, sp.stride)
                pk.max_frames = max(pk.max_frames, total - probe.done[-1])
            self._peek = pk
        pk = self._peek
        pk.planner = self.planner.copy()
        pk.window = [(bufs[t], ld) for bufs, t, ld in zip(self.windows, self.turn, self._ld_prev)]
        pk.pushes = 0
        pk._lstm_started = self._lstm_started
        if self.model.use_rnn and self._lstm_started:
            pk.c_state.copy_(self.c_state)
            pk.h_state.copy_(self.h_state)
        return pk

    def _beam_decoder(self, decode):
        return self._beam_timed if decode == 'beam-timed' else self._beam

    def _beam_check(self, decode):
        if self._beam_mode not in (None, decode):
            raise ValueError(f"decode={decode!r} after decode={self._beam_mode!r} in one utterance: one search sees every frame "
                             '(call reset() to start the next utterance with the other)')
        if self._beam_frames != self.frames_out:
            raise ValueError(f"decode={decode!r} must see every logit frame of the utterance: use it from the first push on (or reset())")

    def _beam_ready(self, decode):
        self._beam_check(decode)
        self._beam_mode = decode
        self._beam_make(decode)

    def _beam_make(self, decode):
        if self._beam_decoder(decode) is None:
            from .ctc import BeamSearchStream
            dec = BeamSearchStream(self.batch, self.beam_width, 0, self.cutoff_top_n, self.device, timesteps=decode == 'beam-timed', **self._lm)
            if decode == 'beam-timed':
                self._beam_timed = dec
            else:
                self._beam = dec

    def _beam_push(self, logits, decode):
        log_probs = hip.ctc_postprocess(logits, None, True, False)[0] if logits.shape[1] else logits
        self._beam_frames += logits.shape[1]
        return self._beam_decoder(decode).push(log_probs)

    def _decode(self, logits):
        tokens, counts = hip.ctc_greedy_stream(logits, self.prev_token)
        tokens, counts = tokens.cpu(), counts.cpu()
        return [tokens[i, : int(counts[i])] for i in range(self.batch)]

    # ---- one step ----------------------------------------------------------------------------------------------------------------
    def _window(self, k, plan, peek=None):
        """Rebuild stage k's window [a, b) into its other buffer; returns the window view.  ``peek``: an uncommitted step -- the pair is not
        flipped, and only the first such step may use the other buffer (``_Peek.destination``)."""
        sp, B = self.specs[k], self.batch
        n_w = plan.b - plan.a
        if n_w > self.caps[k]:
            raise RuntimeError(f'stage {k}: window of {n_w} frames exceeds its capacity {self.caps[k]} (planner bound)')
        ld = hip.round_up4(n_w)
        bufs = self.windows[k]
        if len(bufs) == 1 and plan.n_hist:
            raise RuntimeError(f'stage {k} ({sp.kind}) has no context but retains {plan.n_hist} frames')
        if peek is None:
            old, ld_old = bufs[self.turn[k]], self._ld_prev[k]
            if len(bufs) == 2:
                self.turn[k] ^= 1
            new = bufs[self.turn[k]]
            self._ld_prev[k] = ld
        else:
            old, ld_old = peek.window[k]
            new = peek.destination(k, bufs[len(bufs) - 1 - self.turn[k]])
            peek.window[k] = (new, ld)
        dst = new[: B * sp.c_in * ld].view(B, sp.c_in, ld)
        hist = None
        if plan.n_hist:
            hist = old[: B * sp.c_in * ld_old].view(B, sp.c_in, ld_old)
        src, src_off = self._src
        absmax = self.absmax if (sp.kind == 'dense' and sp.blk > 0) else None
        hip.stream_window(hist, plan.hist_off, plan.n_hist, src, src_off, plan.n_new, dst, absmax)
        return dst, n_w

    def _step(self, chunk, off, n, final, peek=None):
        """One step of the planner on the device; returns its logits.  ``peek`` (a ``_Peek``): the step is not committed -- it runs on the
        peek's planner copy, window table and LSTM state copies, and no field of the session moves."""
        from .executor import node_into
        from .walk import fused_cell
        plans = (self.planner if peek is None else peek.planner).step(n, final)
        m, B = self.model.model, self.batch
        if peek is None:
            self.frames_in += n
        self._src = (chunk, off)                 # (tensor, first column) of the frames the next stage appends to its window
        logits = None
        for k, (sp, plan) in enumerate(zip(self.specs, plans)):
            if plan is None:                     # nothing arrives, nothing is released (a later stage may still release at flush)
                self._src = (None, 0)
                continue
            if sp.kind == 'head' and self.model.use_rnn:
                head = m[sp.layer]
                h = self._src[0]
                logits = torch.empty(B, h.shape[1], head.out_features, device=self.device, dtype=torch.float32)
                hip.linear_head(h, head.weight.detach(), head.bias.detach(), logits)
                break
            win, n_w = self._window(k, plan, peek)
            if not plan.compute:
                self._src = (None, 0)
                continue
            k0 = plan.c - plan.a // sp.stride
            if sp.kind == 'dense':
                conv, norm = m[sp.layer], m[sp.layer + 1]
                t_out = out_length(n_w, sp.stride)
                ld = hip.round_up4(t_out)
                out = self.scratch[: B * sp.c_out * ld].view(B, sp.c_out, ld)
                scheme, packed = self._packed[sp.layer]
                hip.dense_conv1d_fused_packed(win, n_w, packed, sp.c_out, conv.kernel_size, conv.conv.bias.detach(), (), out, conv.strides,
                                              None, scheme, self.absmax if scheme == 'f16x2' else None)
                hip.layernorm_channels(out, norm.weight.detach(), norm.bias.detach(), out, t_out, norm.eps)
                self._src = (out, k0)
            elif sp.kind == 'cell':
                cell = m[sp.layer]
                ld = win.shape[2]
                out = self.scratch[: B * sp.c_out * ld].view(B, sp.c_out, ld)
                nodes = cell.nodes
                groups = getattr(nodes[-1].op, 'groups', 0)
                fused, mask = fused_cell(cell, ld)
                if fused:                        # the executor's one-launch cell (bit-identical to the three node launches)
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
                self._src = (out, k0)
            elif sp.kind == 'lstm':              # no context: the window holds exactly the new frames
                lstm = m[sp.layer]
                nf = n_w
                gates = self.gates[: nf * B * 4 * LSTM_HIDDEN]
                hip.lstm_input_projection_packed(win, nf, self._packed['w_ih'], lstm.bias_ih_l0.detach(), lstm.bias_hh_l0.detach(), gates,
                                                 LSTM_HIDDEN, self.pointwise_ws)
                h = self.h_out[: B * nf * LSTM_HIDDEN].view(B, nf, LSTM_HIDDEN)
                carried = self if peek is None else peek             # (a peek runs from copies: cell_ws is in/out)
                h_state, c_state, cont = carried.h_state[: B * LSTM_HIDDEN], carried.c_state[: B * LSTM_HIDDEN], carried._lstm_started
                hip.lstm_recurrence_frames16_state(gates, self._packed['w_hh16'], c_state, h, self.xcd_ws,
                                                   h_state if cont else None, hip.LSTM_CONTINUE if cont else 0)
                carried._lstm_started = True
                # h_n = the last frame's h becomes the next call's h0 (h_out seen as one row of nf * H floats per utterance)
                hip.stream_window(None, 0, 0, h.view(B, 1, nf * LSTM_HIDDEN), (nf - 1) * LSTM_HIDDEN, LSTM_HIDDEN, h_state.view(B, 1, LSTM_HIDDEN))
                self._src = (h, 0)
            else:                                # head of a model without the LSTM: reads the encoder output's pitched rows
                head = m[sp.layer]
                logits = torch.empty(B, n_w, head.out_features, device=self.device, dtype=torch.float32)
                hip.linear_head_bct(win, n_w, head.weight.detach(), head.bias.detach(), logits)
        if logits is None:
            logits = torch.empty(B, 0, m[self.specs[-1].layer].out_features, device=self.device, dtype=torch.float32)
        if peek is None:
            self.frames_out += logits.shape[1]
        return logits
