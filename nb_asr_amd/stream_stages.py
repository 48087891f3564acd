"""The device side of a streaming session (streaming.py; DESIGN.md 9 "Session and stage engines"): one stage engine per storage type.

``Stages`` holds what a step does in either type -- the buffers every stage needs, the LSTM state and recurrence, the version snapshot
of the packed weights, the window views, ``step`` --, ``StagesF32`` / ``StagesBf16`` what differs: the kernels of the four stage bodies,
the derived weights, where a LayerNorm is applied and how logits are made, joined and read.  A ``StreamingSession`` owns one engine and
hands it the ``_Carried`` record a step advances and the place its windows are built in; the engine never sees the session.

No reference cycle: a dropped session gives its memory back at once, without the cycle collector (a late one shows as allocated
memory in whatever runs next).  So the engine stores no bound method of its own and nothing that closes over itself: its stage table
holds the class's plain functions, and ``StagesF32.linear_ctx`` closes over a dict and a tensor.  Every device tensor sits in an
attribute, list or dict of the engine and is its own allocation (tests/test_stream_launch_sequence_gpu.py finds them so).
"""
import torch

from . import hip
from .streaming import LSTM_HIDDEN, out_length


class Stages:
    """What both storage types share.  Built from (model, specs, caps, batch, device): allocates, packs the weights once."""
    dtype = None                                 # the storage type of windows, scratch and logits
    pointwise_ws_bytes = None                    # the library's workspace rule of the type's pointwise GEMM (`linear` nodes, the LSTM projection)
    cell_mfma = False                            # cells on the matrix cores in one launch: no node scratch

    def __init__(self, model, specs, caps, batch, device):
        from .ops import Linear
        self.model, self.specs, self.caps, self.batch, self.device = model, specs, caps, batch, device
        self.name = str(self.dtype).split('.')[-1]
        self.classes = model.model[specs[-1].layer].out_features
        self.bufs = []                           # every tensor the session owns outside its decoders, streams and listeners
        self.peek_thirds = self.peek_views = None
        self._allocate(any(isinstance(node.op, Linear) for node in model.model[2].nodes))
        # derived weight copies, made once; ``check_params`` refuses to go on once a parameter has changed (its version counter moved)
        self._versions = [(p, p.data_ptr(), p._version) for p in model.parameters()]
        self.packed = {}
        with torch.no_grad():
            self._pack()
        # per stage (its spec, its body, whether it builds a window: not the head behind the LSTM) -- the class's functions, see above
        self._table = [(sp, getattr(type(self), sp.kind), not (sp.kind == 'head' and model.use_rnn)) for sp in specs]

    def buf(self, numel, dtype=torch.float32):
        t = torch.empty(max(int(numel), 4), device=self.device, dtype=dtype)
        self.bufs.append(t)
        return t

    @property
    def state_bytes(self):
        return sum(t.numel() * t.element_size() for t in self.bufs)

    def _allocate(self, has_linear):
        """A pair of windows per stage (the head / LSTM input: one buffer, nothing is retained), scratch for outputs and node results,
        the pointwise workspace, the LSTM's gates, rows and state (``h`` / ``c``: None without it)."""
        model, B, buf, dt, pitch = self.model, self.batch, self.buf, self.dtype, self._pitch
        ws_bytes = getattr(hip.load_library(), self.pointwise_ws_bytes)
        self.windows = []
        out_elems = node_elems = need_pw = 0
        for sp, cap in zip(self.specs, self.caps):
            ld = pitch(cap)
            self.windows.append([buf(*self._window_storage(sp, cap)) for _ in range(2 if sp.kind in ('dense', 'cell') else 1)])
            if sp.kind in ('dense', 'cell'):
                out_elems = max(out_elems, B * sp.c_out * pitch(out_length(cap, sp.stride)))
            if sp.kind == 'cell' and not self.cell_mfma:
                node_elems = max(node_elems, B * sp.c_out * ld)
            if sp.kind == 'lstm' or (sp.kind == 'cell' and has_linear):
                need_pw = max(need_pw, ws_bytes(B, sp.c_in, ld))
        self.scratch = buf(out_elems, dt)
        self.node_scratch = [buf(node_elems, dt), buf(node_elems, dt)] if node_elems else None
        self.pointwise_ws = buf(need_pw, torch.uint8) if need_pw else None
        self.h = self.c = None
        if model.use_rnn:
            lstm_cap = self.caps[[sp.kind for sp in self.specs].index('lstm')]
            self.gates = buf(lstm_cap * B * 4 * LSTM_HIDDEN)
            self.h_out = buf(B * lstm_cap * LSTM_HIDDEN)
            self.h, self.c = buf(B * LSTM_HIDDEN), buf(B * LSTM_HIDDEN)
            self.xcd_ws = buf(hip.lstm_xcd_workspace_bytes(B, LSTM_HIDDEN), torch.uint8)

    def _pitch(self, frames):
        """The row pitch of ``frames`` frames in the engine's storage type."""
        return hip.row_pitch(frames, self.dtype)

    def _window_storage(self, sp, cap):
        """(elements, storage type) of one window buffer of a stage."""
        return self.batch * sp.c_in * self._pitch(cap), self.dtype

    def accepts(self, chunk):
        """Whether ``chunk`` is stored as the first stage's window takes a push's frames: the engine's type, on its device."""
        return chunk.dtype == self.dtype and chunk.device == self.device

    def check_params(self):
        for p, ptr, ver in self._versions:
            if p.data_ptr() != ptr or p._version != ver:
                raise ValueError('a parameter of the model changed after the session packed its weights: create a new session')
        if len(self._versions) != len(list(self.model.parameters())):
            raise ValueError('the model\'s parameters changed after the session packed its weights: create a new session')

    # ---- where a step builds stage k's window: ``place(k, current)``, ``current`` the buffer that holds the stage's window now --------
    def place_other(self, k, current):
        """A committed step and a peek's first push: the pair's other buffer (a one-buffer stage retains nothing: it rebuilds in place)."""
        bufs = self.windows[k]
        return bufs[0] if current is bufs[-1] else bufs[-1]

    def place_third(self, k, current):
        """A peek's second push, whose window the final step still reads: the stage's third buffer."""
        return self.peek_thirds[k]

    def place_peek(self, k, current):
        """A peek's final step, whose windows are consumed by their own stage at once and never retained: the one scratch window, seen
        as the stage's storage type."""
        return self.peek_views[current.dtype]

    def peek_state(self, rec, thirds):
        """What only a peek builds in and advances, made by the first one: the scratch window (sized for the largest stage window), with
        ``thirds`` a third buffer per stage, and (h, c, previous token) of the peek's record, shaped as ``rec``'s."""
        if thirds:
            self.peek_thirds = [torch.empty_like(bufs[0]) for bufs in self.windows]
            self.bufs.extend(self.peek_thirds)
        nbytes = max(bufs[0].numel() * bufs[0].element_size() for bufs in self.windows)
        window = torch.empty(-(-nbytes // 4), device=self.device, dtype=torch.float32)
        self.peek_views = {dt: window if dt == window.dtype else window.view(dt) for dt in {bufs[0].dtype for bufs in self.windows}}
        h, c = (None if t is None else torch.empty_like(t) for t in (rec.h, rec.c))
        prev_token = torch.empty(max(self.batch, 4), device=self.device, dtype=torch.int32)
        self.bufs.extend(t for t in (window, h, c, prev_token) if t is not None)
        return h, c, prev_token[:self.batch]

    def _window_views(self, rec, k, plan, place):
        """(the retained window or None, the new window in the buffer ``place`` names, its frames) of stage k; ``rec`` moves to the new one."""
        sp, B = self.specs[k], self.batch
        n_w = plan.b - plan.a
        if n_w > self.caps[k]:
            raise RuntimeError(f'stage {k}: window of {n_w} frames exceeds its capacity {self.caps[k]} (planner bound)')
        if len(self.windows[k]) == 1 and plan.n_hist:
            raise RuntimeError(f'stage {k} ({sp.kind}) has no context but retains {plan.n_hist} frames')
        old, ld_old = rec.window[k]
        new = place(k, old)
        ld = hip.row_pitch(n_w, new.dtype)
        rec.window[k] = (new, ld)
        dst = new[: B * sp.c_in * ld].view(B, sp.c_in, ld)
        hist = old[: B * sp.c_in * ld_old].view(B, sp.c_in, ld_old) if plan.n_hist else None
        return hist, dst, n_w

    # ---- one step ----------------------------------------------------------------------------------------------------------------
    def step(self, rec, chunk, off, n, final, place):
        """One step of ``rec``'s planner on the device, ``rec`` advanced by it, every new window built where ``place`` says -- which is
        all that tells a committed step from the steps of a peek; returns the step's logits."""
        plans = rec.planner.step(n, final)
        rec.frames_in += n
        out = (chunk, off)                       # (tensor, first column) of the frames the next stage appends to its window
        for k, (sp, body, windowed) in enumerate(self._table):
            plan = plans[k]
            if plan is None:                     # nothing arrives, nothing is released (a later stage may still release at flush)
                out = (None, 0)
                continue
            window = self.window(rec, k, plan, out, place) if windowed else out
            out = body(self, rec, k, sp, plan, window) if plan.compute else (None, 0)      # (not: only the window moves)
        logits = out if isinstance(out, torch.Tensor) else self.logits(0)
        rec.frames_out += logits.shape[1]
        return logits

    # the stage bodies: (record, stage index, spec, plan, (window view, its frames)) -> (tensor, first column) of the outputs kept, or the logits
    def _out(self, sp, ld):
        """A stage's output rows of pitch ``ld`` in the scratch."""
        return self.scratch[: self.batch * sp.c_out * ld].view(self.batch, sp.c_out, ld)

    def _node_by_node(self, nodes, win, n_w, out, *node_args):
        """A cell node by node (``executor.node_into``): the last node writes ``out``, the others take turns in the node scratch."""
        from .executor import node_into
        outs = [win]
        for j, node in enumerate(nodes):
            dst = out if j == len(nodes) - 1 else self.node_scratch[j % 2][: out.numel()].view(out.shape)
            outs.append(node_into(node, outs, n_w, dst, *node_args))

    def _recur(self, rec, gates, nf):
        """The recurrence over ``nf`` frames of gates from the carried (h, c), which it advances; returns (h rows, 0)."""
        B = self.batch
        h = self.h_out[: B * nf * LSTM_HIDDEN].view(B, nf, LSTM_HIDDEN)
        h_state, c_state, cont = rec.h[: B * LSTM_HIDDEN], rec.c[: B * LSTM_HIDDEN], rec.lstm_started
        hip.lstm_recurrence_frames16_state(gates, self.packed['w_hh16'], c_state, h, self.xcd_ws,
                                           h_state if cont else None, hip.LSTM_CONTINUE if cont else 0)
        rec.lstm_started = True
        # h_n = the last frame's h becomes the next call's h0 (h_out seen as one row of nf * H floats per utterance)
        hip.stream_window(None, 0, 0, h.view(B, 1, nf * LSTM_HIDDEN), (nf - 1) * LSTM_HIDDEN, LSTM_HIDDEN, h_state.view(B, 1, LSTM_HIDDEN))
        return h, 0

    def head(self, rec, k, sp, plan, source):
        head = self.model.model[sp.layer]
        weight, bias = self._f32(head.weight), self._f32(head.bias)
        if self.model.use_rnn:                   # the LSTM's (batch, frames, hidden) rows, no window
            h = source[0]
            return self._logits_of(h.shape[1], lambda out: hip.linear_head(h, weight, bias, out))
        win, n_w = source                        # without the LSTM: the encoder output's pitched float32 rows
        return self._logits_of(n_w, lambda out: hip.linear_head_bct(win, n_w, weight, bias, out))

    # ---- logits ------------------------------------------------------------------------------------------------------------------
    def logits(self, frames):
        return torch.empty(self.batch, frames, self.classes, device=self.device, dtype=self.dtype)

    def join(self, outs):
        """The logits of several steps as one tensor."""
        return outs[0] if len(outs) == 1 else self._cat(outs)


class StagesF32(Stages):
    """The float32 session: the whole forward's fp32 kernels, every LayerNorm applied by the stage it follows."""
    dtype = torch.float32
    pointwise_ws_bytes = 'nbasr_pointwise_workspace_bytes'
    _f32 = staticmethod(torch.Tensor.detach)     # a parameter as the kernels read it

    def _allocate(self, has_linear):
        super()._allocate(has_linear)
        self.absmax = self.buf(self.batch)[:self.batch]

    def _pack(self):
        import torch.nn as nn
        from .ops import PadConvRelu, Linear
        m, packed, ws = self.model.model, self.packed, self.pointwise_ws
        for sp in self.specs:
            if sp.kind == 'dense':
                conv = m[sp.layer]
                scheme = 'bf16x3' if sp.blk == 0 else 'f16x2'
                packed[sp.layer] = (scheme, hip.pack_dense_weights(conv.conv.weight.detach(), conv.strides, scheme))
            elif sp.kind == 'cell':
                for node in m[sp.layer].nodes:
                    if isinstance(node.op, PadConvRelu):
                        packed[id(node.op)] = hip.pack_grouped_weights(node.op.conv.weight.detach().contiguous(), node.op.groups)
                    elif isinstance(node.op, Linear):
                        packed[id(node.op.linear)] = hip.pack_pointwise_weights(node.op.linear.weight.detach())
            elif sp.kind == 'lstm':
                lstm = m[sp.layer]
                assert isinstance(lstm, nn.LSTM)
                packed['w_ih'] = hip.pack_pointwise_weights(lstm.weight_ih_l0.detach())
                packed['w_hh16'] = hip.lstm_pack_whh16(lstm.weight_hh_l0.detach().contiguous())
        self.bufs.extend(v[1] if isinstance(v, tuple) else v for v in packed.values())
        # node_into's (packed weights of a `linear` op, workspace) lookups, made once: over the dict and the tensor, not over the engine
        self.linear_ctx = (lambda lin: packed[id(lin)], lambda c_in, ld: ws)

    def window(self, rec, k, plan, src, place):
        """Build stage k's window [a, b) from the retained frames of its current one and the new frames at ``src`` = (tensor, first
        column), in the buffer ``place`` names; returns (the window view, its frames)."""
        sp = self.specs[k]
        hist, dst, n_w = self._window_views(rec, k, plan, place)
        absmax = self.absmax if (sp.kind == 'dense' and sp.blk > 0) else None
        hip.stream_window(hist, plan.hist_off, plan.n_hist, src[0], src[1], plan.n_new, dst, absmax)
        return dst, n_w

    def dense(self, rec, k, sp, plan, window):
        win, n_w = window
        conv, norm = self.model.model[sp.layer], self.model.model[sp.layer + 1]
        t_out = out_length(n_w, sp.stride)
        out = self._out(sp, self._pitch(t_out))
        scheme, packed = self.packed[sp.layer]
        hip.dense_conv1d_fused_packed(win, n_w, packed, sp.c_out, conv.kernel_size, conv.conv.bias.detach(), (), out, conv.strides,
                                      None, scheme, self.absmax if scheme == 'f16x2' else None)
        hip.layernorm_channels(out, norm.weight.detach(), norm.bias.detach(), out, t_out, norm.eps)
        return out, plan.c - plan.a // sp.stride

    def cell(self, rec, k, sp, plan, window):
        from .walk import fused_cell
        win, n_w = window
        cell = self.model.model[sp.layer]
        ld = win.shape[2]
        out = self._out(sp, ld)
        nodes = cell.nodes
        fused, mask = fused_cell(cell, ld)
        if fused:                                # the executor's one-launch cell (bit-identical to the three node launches)
            specs = [(self.packed[id(nd.op)], nd.op.conv.bias.detach(), nd.op.kernel_size, nd.op.dilation) for nd in nodes]
            hip.grouped_cell_fused(win, specs, mask, out, n_w, nodes[-1].op.groups)
        else:
            self._node_by_node(nodes, win, n_w, out, None, None, self.linear_ctx, 0)
        if cell.use_norm:
            norm = cell.norm_layer
            hip.layernorm_channels(out, norm.weight.detach(), norm.bias.detach(), out, n_w, norm.eps)
        return out, plan.c - plan.a

    def lstm(self, rec, k, sp, plan, window):
        win, nf = window                         # no context: the window holds exactly the new frames
        lstm = self.model.model[sp.layer]
        gates = self.gates[: nf * self.batch * 4 * LSTM_HIDDEN]
        hip.lstm_input_projection_packed(win, nf, self.packed['w_ih'], lstm.bias_ih_l0.detach(), lstm.bias_hh_l0.detach(), gates,
                                         LSTM_HIDDEN, self.pointwise_ws)
        return self._recur(rec, gates, nf)

    def _logits_of(self, frames, head_into):
        return head_into(self.logits(frames))

    @staticmethod
    def _cat(outs):
        return torch.cat(outs, 1)

    @staticmethod
    def heard(logits):
        """What the decoders and listeners read: the logits themselves."""
        return logits


class StagesBf16(Stages):
    """The bfloat16 session: bf16 rows pitched to 8 frames in front of every encoder stage and the LSTM (fp32 rows in front of a head
    without LSTM: the last LayerNorm writes fp32), bf16 scratch, the bf16 matrix-core kernels with every LayerNorm where
    ``walk.WalkBf16`` places it (``_pack``); LayerNorm statistics, gates, h, c and the logits ahead of their one rounding in fp32.
    It is also what ``executor.node_into(..., copies=)`` reads a bf16 forward's derived weights from: the four lookups of a
    ``ForwardPlan`` it uses, answered from what the engine packed once."""
    dtype = torch.bfloat16
    pointwise_ws_bytes = 'nbasr_pointwise_bf16_workspace_bytes'

    def _f32(self, param):
        return self.kept[id(param)]

    def _packed_grouped(self, op):
        return self.packed[id(op)]

    def _packed_linear_bf16(self, w):
        return self.packed[id(w)]

    def _pointwise_bf16_ws(self, batch, c_in, ld):
        return self.pointwise_ws

    def _allocate(self, has_linear):
        """Fixes what must not depend on a push's frame count: whether the cells run on the matrix cores (they do where the stage's
        largest window fits; else every window takes the node launches)."""
        from .walk import _CELL_SKIPS
        from .ops import PadConvRelu, Identity
        model, caps, B, buf, pitch = self.model, self.caps, self.batch, self.buf, self._pitch
        cells = [(sp, pitch(cap)) for sp, cap in zip(self.specs, caps) if sp.kind == 'cell']
        nodes = model.model[cells[0][0].layer].nodes
        conv_only = len(nodes) == 3 and all(isinstance(n.op, PadConvRelu) and n.op.groups > 1 for n in nodes)
        self.cell_mfma = conv_only and all(hip.grouped_cell_mfma_fits(sp.c_in, ld, model.model[sp.layer].nodes[-1].op.groups) for sp, ld in cells)
        self._skip_mask = sum(1 << bit for bit, (j, i) in enumerate(_CELL_SKIPS) if isinstance(nodes[j].branch_ops[i], Identity)) if conv_only else 0
        super()._allocate(has_linear)
        image_bytes = hip.load_library().nbasr_bf16_image_bytes
        self.stats = buf(B * 2 * pitch(max(caps)))           # per-frame (mean, rstd) of the LayerNorm a stage applies while it loads its window
        self.image = buf(max([16] + [image_bytes(B, sp.c_in, pitch(cap)) for sp, cap in zip(self.specs, caps) if sp.kind == 'dense']), torch.uint8)
        self.logits32 = buf(hip.round_up8(B * max(caps[-2:]) * self.classes))
        if not model.use_rnn:
            sp, ld = cells[-1]
            self.enc32 = buf(B * sp.c_out * ld)  # the encoder output as the head reads it

    def _window_storage(self, sp, cap):
        if sp.kind != 'head':
            return super()._window_storage(sp, cap)
        return (0 if self.model.use_rnn else self.batch * sp.c_in * hip.row_pitch(cap)), torch.float32    # behind the LSTM: no window

    def _pack(self):
        """The operand images the matrix-core kernels take (packed from fp32 copies that are dropped again) and fp32 copies of what the
        kernels read as fp32 -- biases, gamma / beta, the head (``kept``, by ``id(parameter)``).  Also settles, per stage, where its
        LayerNorm is applied (``walk.WalkBf16``'s placement): ``_ln_in[k]`` = (gamma, beta, eps) of the LayerNorm stage k applies while
        it loads its un-normalised window, ``_ln_out[k]`` = (how, gamma, beta, eps) of the one it applies to its output ('inplace':
        bf16 rows for a cell that starts with `linear`; 'f32': fp32 rows for the head, gamma None: only widened)."""
        import torch.nn as nn
        from . import tiles
        from .ops import PadConvRelu, Linear
        from .walk import cheap_consumer
        m, B, packed = self.model.model, self.batch, self.packed
        kept = self.kept = {}

        def f32(p):
            return p.detach().float().contiguous()

        def keep(p):
            if id(p) not in kept:
                kept[id(p)] = f32(p)
            return kept[id(p)]

        norms = [None] * len(self.specs)         # the LayerNorm behind each stage
        for k, (sp, cap) in enumerate(zip(self.specs, self.caps)):
            if sp.kind == 'dense':
                conv, norms[k] = m[sp.layer], m[sp.layer + 1]
                # the row tile of the stage's largest window, for every push: one packed image (every tiling gives the same bits)
                rows, ftile = tiles.bf16_tile(B, sp.c_out, out_length(cap, sp.stride))
                packed[sp.layer] = (hip.pack_dense_weights_bf16(f32(conv.conv.weight), conv.strides, rows), rows, ftile)
                keep(conv.conv.bias)
            elif sp.kind == 'cell':
                cell = m[sp.layer]
                norms[k] = cell.norm_layer if cell.use_norm else None
                for node in cell.nodes:
                    op = node.op
                    if isinstance(op, PadConvRelu):
                        w = f32(op.conv.weight)
                        packed[id(op)] = hip.grouped_cell_mfma_pack(w, op.groups) if self.cell_mfma else hip.pack_grouped_weights(w, op.groups)
                        keep(op.conv.bias)
                    elif isinstance(op, Linear):
                        packed[id(op.linear.weight)] = hip.pack_pointwise_weights_bf16(f32(op.linear.weight))
                        keep(op.linear.bias)
            elif sp.kind == 'lstm':
                lstm = m[sp.layer]
                assert isinstance(lstm, nn.LSTM)
                packed['w_ih'] = hip.pack_pointwise_weights_bf16(f32(lstm.weight_ih_l0))
                packed['w_hh16'] = hip.lstm_pack_whh16(f32(lstm.weight_hh_l0))
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
            elif norm is not None:               # a conv-only cell, a dense conv's operand image, the LSTM's projection: on load
                self._ln_in[k + 1] = affine
        self.bufs.extend(kept.values())
        self.bufs.extend(v[0] if isinstance(v, tuple) else v for v in packed.values())

    def window(self, rec, k, plan, src, place):
        """``StagesF32.window`` for bfloat16 rows (pitch: 8 frames; no range bound); ``src`` is bfloat16, or the front-end's float32
        frames at stage 0.  The head without the LSTM reads float32 rows, built as the float32 session builds them."""
        hist, dst, n_w = self._window_views(rec, k, plan, place)
        build = hip.stream_window if self.specs[k].kind == 'head' else hip.stream_window_bf16
        build(hist, plan.hist_off, plan.n_hist, src[0], src[1], plan.n_new, dst)
        return dst, n_w

    def _pending(self, k, win):
        """(stats, gamma, beta) of the LayerNorm stage k applies while it loads ``win``, its per-frame statistics taken by the caller
        (one read pass; per frame, so the chunking does not reach them), and its eps; (None, 0.0) where the window holds normalised rows."""
        if self._ln_in[k] is None:
            return None, 0.0
        gamma, beta, eps = self._ln_in[k]
        B, _, ld = win.shape
        return (self.stats[: B * 2 * ld].view(B, 2, ld), gamma, beta), eps

    def _norm_out(self, k, out, frames):
        """Stage k's own LayerNorm, where it is not left to the consumer's load: in place, or as the fp32 rows the head reads."""
        if self._ln_out[k] is None:
            return out
        how, gamma, beta, eps = self._ln_out[k]
        if how == 'inplace':
            return hip.layernorm_channels(out, gamma, beta, out, frames, eps)
        enc = self.enc32[: out.numel()].view(out.shape)
        return hip.convert(out, enc) if gamma is None else hip.layernorm_channels(out, gamma, beta, enc, frames, eps)

    def dense(self, rec, k, sp, plan, window):
        win, n_w = window
        conv = self.model.model[sp.layer]
        t_out = out_length(n_w, sp.stride)
        out = self._out(sp, self._pitch(t_out))
        ln, eps = self._pending(k, win)          # (the image pass fills the statistics itself)
        image = hip.bf16_image(win, self.image, n_w, ln and ln[1:], ln and ln[0], eps)
        packed, rows, ftile = self.packed[sp.layer]
        hip.dense_conv1d_bf16_img(image, self.batch, sp.c_in, n_w, win.shape[2], packed, sp.c_out, conv.kernel_size, self._f32(conv.conv.bias), out,
                                  conv.strides, rows, ftile)
        return self._norm_out(k, out, t_out), plan.c - plan.a // sp.stride

    def cell(self, rec, k, sp, plan, window):
        win, n_w = window
        out = self._out(sp, win.shape[2])
        ln0, eps = self._pending(k, win)
        if ln0 is not None:
            hip.channel_stats(win, ln0[0], n_w, eps)
        nodes = self.model.model[sp.layer].nodes
        if self.cell_mfma:
            specs = [(self.packed[id(nd.op)], self._f32(nd.op.conv.bias), nd.op.kernel_size, nd.op.dilation) for nd in nodes]
            hip.grouped_cell_mfma(win, specs, self._skip_mask, out, n_w, nodes[-1].op.groups, ln0)
        else:                                    # one variant for every window: GC_FPL8 is the whole forward's choice for long rows
            self._node_by_node(nodes, win, n_w, out, ln0, None, None, hip.GC_WPERM, self)
        return self._norm_out(k, out, n_w), plan.c - plan.a

    def lstm(self, rec, k, sp, plan, window):
        win, nf = window                         # un-normalised bf16 rows: the projection applies the last cell's LayerNorm on load
        lstm, f32 = self.model.model[sp.layer], self._f32
        ln, eps = self._pending(k, win)
        if ln is not None:
            hip.channel_stats(win, ln[0], nf, eps)
        gates = self.gates[: nf * self.batch * 4 * LSTM_HIDDEN]
        hip.lstm_input_projection_bf16(win, nf, self.packed['w_ih'], f32(lstm.bias_ih_l0), f32(lstm.bias_hh_l0), gates, LSTM_HIDDEN,
                                       self.pointwise_ws, ln)
        return self._recur(rec, gates, nf)

    def _logits_of(self, frames, head_into):
        """The head's fp32 logits (``head_into(out)`` writes them) rounded once to bfloat16, in whole 8-element chunks as ``WalkBf16.head``
        does: the last chunk's padding is converted too and never returned."""
        logits = self._rounded(frames)
        n8 = logits.nbasr_flat.numel()
        head_into(self.logits32[: logits.numel()].view(logits.shape))
        hip.convert(self.logits32[:n8], logits.nbasr_flat)
        return logits

    def _rounded(self, frames):
        """(batch, frames, classes) bfloat16 logits over a buffer of whole 8-element chunks (``nbasr_flat``): what nbasr_convert works in."""
        n = self.batch * frames * self.classes
        flat = torch.empty(max(hip.round_up8(n), 8), device=self.device, dtype=self.dtype)
        logits = flat[:n].view(self.batch, frames, self.classes)
        logits.nbasr_flat = flat
        return logits

    def _cat(self, outs):
        """Over a buffer padded to 8 elements (``nbasr_flat``), as a step's logits are."""
        frames = sum(o.shape[1] for o in outs)
        return torch.cat(outs, 1, out=self._rounded(frames)) if frames else outs[0]

    def heard(self, logits):
        """What the decoders and listeners read: the logits' fp32 widening (one nbasr_convert, made once per result), so that every
        decode result is the offline function's on ``logits.float()``."""
        wide = getattr(logits, 'nbasr_wide', None)
        if wide is None:
            if logits.shape[1] == 0:
                wide = torch.empty(logits.shape, device=self.device, dtype=torch.float32)
            else:
                flat = logits.nbasr_flat
                wide = hip.convert(flat, torch.empty(flat.shape, device=self.device, dtype=torch.float32))[:logits.numel()].view(logits.shape)
            logits.nbasr_wide = wide
        return wide
