"""The launch sequence of one forward: a walk over ``model.model`` that calls one step per layer kind.

``executor.ForwardPlan`` owns what outlives a call -- workspaces, derived weight copies, the recurrence, tapes, graphs; the tile and kernel-variant
choices are the free functions of ``tiles.py``.  A
``Walk`` is what ONE forward knows about the activation it is carrying: where it lives, whether a LayerNorm is still pending on it, what
by-product the last producer left (a range bound or an operand image from a LayerNorm, statistics partials from a dense convolution), which
block it is in, and whether the tail has moved to the side stream.  It dies with the call, so nothing of an aborted forward reaches the next one.

One dispatch loop (``Walk.run``) and the steps that do not depend on the storage type live in ``Walk``; ``WalkF32`` and ``WalkBf16`` hold the
steps that do: fp32 rows with a range bound or a split-fp16 operand image against bf16 rows with a one-term image, fp32 copies of the
parameters, the matrix-core cell, the hand-over to the fp32 tail and the conversion of the logits.  Every step reads its inputs into locals
before it hands a closure to ``plan._timed``: nothing a closure sees is re-bound afterwards.
"""
import torch
import torch.nn as nn

from . import hip, tiles
from .executor import PendingLogits, node_into
from .ops import PadConvRelu, Linear, Identity

_NODE_KINDS = {'PadConvRelu': 'grouped_conv', 'Linear': 'linear_op', 'Zero': 'skip_sum'}
_CELL_SKIPS = ((0, 0), (1, 0), (1, 1), (2, 0), (2, 1), (2, 2))      # (node, input) behind bits 0-5 of a fused cell's skip mask


def cheap_consumer(nxt):
    """Deferral pays only where normalising on load is nearly free: a following cell whose first node is a grouped
    convolution (or `zero`).  GEMM consumers (the next block's dense conv, a `linear` first node, the LSTM, the head)
    stage their input through a register pipeline where the extra per-element work costs more than the LayerNorm
    pass it saves (measured: +2 ms on the dense convs, +1.2 ms on the LSTM projection)."""
    from .model import SearchCell
    return isinstance(nxt, SearchCell) and not isinstance(nxt.nodes[0].op, Linear)


def fused_cell(cell, ld):
    """(groups per statistics partial, skip mask) where ``cell`` can run as ONE launch on rows of pitch ``ld`` -- three grouped
    convolutions and a row that fits a workgroup (grouped_cell.hip) --, else (0, 0)."""
    nodes = cell.nodes
    if len(nodes) != 3 or not all(isinstance(n.op, PadConvRelu) and n.op.groups > 1 for n in nodes):
        return 0, 0
    gpp = hip.grouped_cell_fits(cell.filters, ld, nodes[-1].op.groups)
    if not gpp:
        return 0, 0
    return gpp, sum(1 << bit for bit, (j, i) in enumerate(_CELL_SKIPS) if isinstance(nodes[j].branch_ops[i], Identity))


def skip_count(node):
    return sum(isinstance(branch, Identity) for branch in node.branch_ops)


class Walk:
    """State of one forward and the steps both storage types share."""
    dtype = None
    copies = None             # node_into: the plan whose fp32 / re-laid-out parameter copies the node kernels read (bf16 storage)
    lin_ctx = None            # node_into: fp32 `linear` ops on the fp16 matrix cores

    def __init__(self, plan, model, x, taps, pipelined, capturing, group=None):
        self.plan, self.layers, self.taps = plan, model.model, taps
        self.pipelined, self.capturing, self.group = bool(pipelined), capturing, group
        self.pipe = self.pipelined and model.use_rnn and taps is None and plan._tail_on_side_stream(x.shape[0])
        if not self.pipe and not capturing:
            # the plain path shares the gate / cell / h buffers with pipelined tails that may still be running
            plan.wait_tails()
        plan._set_shape(x.shape[0], x.shape[2], model.use_rnn, x.dtype)
        self.act, self.frames, self.cur = x, plan.frames, None      # `cur`: pool slot holding `act` (None: the caller's x, a hand-over copy)
        self.pending = None           # (stats, gamma, beta) while `act` still awaits its LayerNorm
        self.absmax = None            # (B,) bounds of max|act[b]| when a LayerNorm has just written `act` together with them
        self.image = None             # the operand image a LayerNorm (or the bf16 input pass) wrote for the dense convolution behind it
        self.conv_part = None         # statistics partials the dense convolution that wrote `act` left for the LayerNorm behind it
        self.blk = -1
        self.stat_turn = 0
        self.tail_slot, self.tail_ctx = None, None      # pipelined tail: its double-buffer slot / the side-stream context once entered
        self.logits = None

    def run(self):
        from .model import SearchCell
        steps = ((PadConvRelu, self.dense), (nn.LayerNorm, self.block_norm), (SearchCell, self.cell), (nn.Dropout, self.dropout),
                 (nn.LSTM, self.lstm), (nn.Linear, self.head))
        try:
            for idx, layer in enumerate(self.layers):
                step = next((step for kind, step in steps if isinstance(layer, kind)), None)
                if step is None:
                    raise TypeError(f'unsupported layer {type(layer).__name__} in the model list')
                handle = step(idx, layer)
                if handle is not None:                  # a member of a tail group ends at the LSTM (group_tail)
                    return handle
            return self.finish()
        except BaseException:
            if self.tail_ctx is not None:               # do not leave the caller on the side stream
                self.tail_ctx.__exit__(None, None, None)
            raise

    # ---- helpers, each written once ----------------------------------------------------------------------------------------
    def layer_at(self, idx):
        return self.layers[idx] if idx < len(self.layers) else None

    def consumers(self, idx):
        """(the layer behind layer ``idx``, the one that really reads its output: dropout is the identity here)."""
        nxt = self.layer_at(idx + 1)
        return nxt, (self.layer_at(idx + 2) if isinstance(nxt, nn.Dropout) else nxt)

    def next_stats(self):
        """The statistics slot the NEXT pending LayerNorm uses: the two turn, so a cell's nodes still read one while its last node fills the other."""
        self.stat_turn ^= 1
        b, _, ld = self.act.shape
        return self.plan.stats[self.stat_turn][: b * 2 * ld].view(b, 2, ld)

    def tap(self, idx):
        if self.taps is None:
            return
        if self.act is self.plan.h_out:
            self.taps[idx] = self.act.permute(0, 2, 1).clone()              # (B, H, T) like the oracle's LSTM tap
        else:
            self.taps[idx] = self.act[:, :, :self.frames].clone()

    def tap_normalised(self, idx, gamma, beta, eps):
        """Parity debugging: materialise a normalised copy for the tap, the flow stays deferred."""
        if self.taps is not None:
            copy = torch.empty_like(self.act)
            hip.layernorm_channels(self.act, gamma, beta, copy, self.frames, eps)
            self.taps[idx] = copy[:, :, :self.frames].clone()

    def defer_norm(self, idx, norm, meta, partials):
        """Leave ``norm`` pending on `act`: only its statistics are computed now.  ``partials`` = (workspace, groups, groups per partial)
        when the kernel that wrote `act` left partial statistics -- merging them is a few rows per utterance -- else a read pass over `act`."""
        gamma, beta = self.f32(norm.weight), self.f32(norm.bias)
        stats, act, frames, eps = self.next_stats(), self.act, self.frames, norm.eps
        if partials is not None:
            ws, groups, per_part = partials
            self.plan._timed('stats_finalize', meta, lambda: hip.grouped_stats_finalize(ws, stats, act.shape[1], frames, groups, eps, per_part))
        else:
            self.plan._timed('channel_stats', meta, lambda: hip.channel_stats(act, stats, frames, eps))
        self.pending = (stats, gamma, beta)
        self.tap_normalised(idx, gamma, beta, eps)

    def norm_meta(self):
        return (self.blk, self.act.shape[1], self.act.shape[1], 0, self.frames, 0)

    def enter_tail(self):
        """Everything from here on runs on the side stream."""
        self.plan._to_side_stream()
        self.tail_ctx = torch.cuda.stream(self.plan.side_stream)
        self.tail_ctx.__enter__()

    def leave_tail(self):
        self.plan._tail_enqueued(self.tail_slot)
        ctx, self.tail_ctx = self.tail_ctx, None
        ctx.__exit__(None, None, None)

    def finish(self):
        on_side = self.tail_ctx is not None
        if on_side:
            self.leave_tail()
        if self.logits is None:
            raise RuntimeError('the model list does not end in the CTC head')
        if self.pipelined:
            return PendingLogits(self.logits, self.plan.tail_done[self.tail_slot] if on_side else None)
        if self.taps is not None:
            self.taps[len(self.layers) - 1] = self.logits.clone()
        return self.logits

    # ---- steps --------------------------------------------------------------------------------------------------------------
    def dense(self, idx, layer):
        plan, conv = self.plan, layer.conv
        self.blk += 1
        dst = 0 if self.cur != 0 else 1
        t_out = plan.block_frames[self.blk]
        out = plan._view(dst, conv.out_channels, t_out, self.dtype)
        part = self.dense_conv(idx, layer, out, t_out, (self.blk, conv.in_channels, conv.out_channels, layer.kernel_size, t_out, 0))
        self.act, self.frames, self.cur = out, t_out, dst
        self.pending = self.absmax = self.image = None
        self.conv_part = part
        self.tap(idx)

    def block_norm(self, idx, layer):
        if self.act.dim() != 3 or self.pending is not None:
            raise RuntimeError('LayerNorm in an unexpected position of the layer list')
        partials, self.conv_part = self.conv_part, None
        if partials is not None:                        # one (mean, M2) row pair per DENSE_STATS_UNIT channels: every channel its own group
            partials = (partials, self.act.shape[1], hip.DENSE_STATS_UNIT)
        self.norm(idx, layer, *self.consumers(idx), partials)

    def cell(self, idx, layer):
        plan, nodes = self.plan, layer.nodes
        free = [i for i in range(4) if i != self.cur]
        if len(nodes) > len(free):
            raise NotImplementedError(f'cells with {len(nodes)} nodes need a larger buffer pool')
        nxt, after = self.consumers(idx)
        # a deferred cell LayerNorm whose producer is a grouped conv gets its statistics from that launch's epilogue (no pass over the tensor)
        last_op = nodes[-1].op
        want_stats = layer.use_norm and self.defers(nxt, after) and isinstance(last_op, PadConvRelu) and last_op.groups > 1
        gpp, mask = fused_cell(layer, self.act.shape[2]) if plan.cell_fusion else (0, 0)
        if gpp:
            out = plan._view(free[2], layer.filters, self.frames, self.dtype)
            want_stats = self.fused(layer, mask, out, want_stats)
        else:
            outs = [self.act]
            for j, (node, dst) in enumerate(zip(nodes, free)):
                stats = (None, plan.stats_ws, layer.norm_layer.eps) if want_stats and j == len(nodes) - 1 else None
                outs.append(self.node(layer, node, outs, plan._view(dst, layer.filters, self.frames, self.dtype), stats))
            out = outs[-1]
        self.act, self.cur, self.pending = out, free[len(nodes) - 1], None
        partials = (plan.stats_ws, last_op.groups, gpp or 4) if want_stats else None
        self.after_cell(idx, layer.norm_layer if layer.use_norm else None, nxt, after, partials)

    def fused(self, layer, mask, out, want_stats):
        """The cell as ONE launch: x1 and x2 never touch HBM, and with ``want_stats`` the statistics partials of the result come out of the
        same launch.  Bit-identical to the three node launches.  Returns whether the launch left partials."""
        plan, nodes = self.plan, layer.nodes
        biases = [self.f32(n.op.conv.bias) for n in nodes]
        specs = [(plan._packed_grouped(n.op), bias, n.op.kernel_size, n.op.dilation) for n, bias in zip(nodes, biases)]
        src, frames, ln0, groups, ws = self.act, self.frames, self.pending, nodes[-1].op.groups, plan.stats_ws if want_stats else None
        plan._timed('grouped_cell', self.fused_meta(layer), lambda: hip.grouped_cell_fused(src, specs, mask, out, frames, groups, ln0, ws))
        return want_stats

    def fused_meta(self, layer):
        return (self.blk, layer.filters, tuple(n.op.kernel_size for n in layer.nodes), tuple(skip_count(n) for n in layer.nodes), self.frames, 0)

    def node(self, layer, node, outs, out, stats):
        """One node launch: ``out = op(outs[-1]) + flagged earlier outputs``; the pending LayerNorm of the cell input rides along (node_into)."""
        plan, frames, ln0 = self.plan, self.frames, self.pending
        meta = (self.blk, layer.filters, layer.filters, getattr(node.op, 'kernel_size', 1), frames, skip_count(node))
        variant = self.gc_variant(out, node, ln0, stats, len(outs))
        return plan._timed(_NODE_KINDS.get(type(node.op).__name__), meta,
                           lambda: node_into(node, outs, frames, out, ln0, stats, self.lin_ctx, variant, self.copies))

    def dropout(self, idx, layer):
        if self.taps is not None:                       # identity: eval mode or p == 0 (checked by the model)
            self.taps[idx] = self.taps[idx - 1]

    def lstm(self, idx, layer):
        plan = self.plan
        b_ih, b_hh = self.f32(layer.bias_ih_l0), self.f32(layer.bias_hh_l0)
        meta = (self.blk, layer.input_size, layer.hidden_size, 0, self.frames, 0)
        if self.group is not None:
            return self.group_tail(idx, layer, b_ih, b_hh, meta)
        # the input projection is one large GEMM: it stays with the encoder; only the recurrence moves over
        gates = plan.gates_pipe[self.tail_slot] if self.pipe else plan.gates_ws
        self.project(layer, b_ih, b_hh, gates, meta)
        if self.pipe:
            self.enter_tail()
        pipe, capturing = self.pipe, self.capturing
        plan._timed('lstm', meta, lambda: plan._recurrence(gates, layer.weight_hh_l0, layer.hidden_size, pipe, capturing))
        self.act, self.pending = plan.h_out, None       # (batch, frames, hidden)
        self.tap(idx)

    def project_packed(self, layer, b_ih, b_hh, gates, meta, **into):
        """The LSTM's input projection of fp32 rows on the fp16 matrix cores; a pending LayerNorm is applied while the operand is split."""
        plan, src, frames, ln = self.plan, self.act, self.frames, self.pending
        packed_ih, ws = plan._packed_linear(layer.weight_ih_l0), plan._pointwise_ws(src.shape[1], src.shape[2])
        plan._timed('lstm_projection', meta, lambda: hip.lstm_input_projection_packed(src, frames, packed_ih, b_ih, b_hh, gates, layer.hidden_size,
                                                                                      ws, ln, **into))

    def head_into(self, layer, out):
        weight, bias = self.f32(layer.weight), self.f32(layer.bias)
        if self.act is self.plan.h_out:
            hip.linear_head(self.act, weight, bias, out)
        else:
            hip.linear_head_bct(self.act, self.frames, weight, bias, out, self.pending)


class WalkF32(Walk):
    """fp32 rows (pitch: 4 frames).  A LayerNorm in front of a dense convolution leaves the range bound or the split-fp16 operand image of
    its output; parameters are read where they are."""
    dtype = torch.float32

    def __init__(self, plan, model, x, taps, pipelined, capturing, group=None):
        super().__init__(plan, model, x, taps, pipelined, capturing, group)
        if plan.dense_mode != 'f32' and (x.shape[-1] % 4 or x.data_ptr() % 16):
            # the packed dense conv fetches aligned 4-frame quads: bring a ragged-length input into the pitched layout
            self.cur = 2
            self.act = hip.repitch(x, plan._view(2, x.shape[1], plan.frames), plan.frames)
        self.input_range = None
        if plan.dense_mode == 'auto' and x.shape[0] > 0:
            # the model input is caller data: one small reduction gives the first conv its range AND decides, per utterance
            # and on the device, whether that range is tame enough for the scaled fp16 scheme (nbasr.h: nbasr_input_range)
            self.input_range = hip.input_range(self.act, self.frames, plan._buf('input_range', 4 * x.shape[0])[: 4 * x.shape[0]])
        self.lin_ctx = (plan._packed_linear, plan._pointwise_ws) if plan.linear_mode == 'f16x2' else None

    @staticmethod
    def f32(param):
        return param.detach()

    def gc_variant(self, view, node, ln0, stats, n_inputs):
        return tiles.gc_variant(tiles._GC_TABLE, view.shape, node, ln0, stats, n_inputs)

    def defers(self, nxt, after):
        # the LSTM's input projection pre-splits its operand in a streaming pass that applies a pending LayerNorm while loading
        # (gemm_pointwise.hip, PwF16x2), and it runs on the MAIN stream in both modes: the cell in front of it defers its LayerNorm like a
        # cell in front of a grouped conv does -- no materialised copy of the encoder output
        return cheap_consumer(nxt) or (isinstance(after, nn.LSTM) and self.plan.linear_mode == 'f16x2')

    def dense_conv(self, idx, layer, out, t_out, meta):
        """``self.absmax``: bounds of max|act[b]| when `act` was just written by the LayerNorm kernel; ``self.image`` = (image, bound): the
        LayerNorm of `act` was written as the pre-split operand image instead.  Returns the statistics partials the launch left."""
        plan, conv, blk = self.plan, layer.conv, self.blk
        src, frames, ln, absmax = self.act, self.frames, self.pending, self.absmax
        bias = conv.bias.detach()
        # the block LayerNorm behind this convolution is deferred into the next cell's load: its statistics then come out of the
        # convolution's own epilogue (round 5) instead of a pass over the output
        # (the finalize kernel merges <= 128 partial rows: wider than 128 x 16 channels falls back to the statistics pass)
        want_stats = (plan.conv_stats and isinstance(self.layer_at(idx + 1), nn.LayerNorm) and cheap_consumer(self.layer_at(idx + 2))
                      and layer.kernel_size == 8 and -(-conv.out_channels // hip.DENSE_STATS_UNIT) <= 128)

        def partials():
            return plan._dense_part(conv.out_channels, out.shape[2]) if want_stats else None
        rng, self.input_range = self.input_range, None
        if rng is not None and layer.kernel_size == 8 and ln is None and self.image is None:
            # fp16 split with per-utterance fall-back to bf16x3 (extreme / non-finite input); image path: one split
            # pass over the input, then the same DMA-only GEMM as convs 1-3
            b, c, ld = src.shape
            image = plan._buf('input_image', max(hip.load_library().nbasr_split_image_bytes(b, c, ld), 16), torch.uint8)
            rows, ftile = tiles.dense_tile(plan.batch, conv.in_channels, conv.out_channels, layer.strides, t_out)
            plan.dense_row_tiles[blk], plan.dense_frame_tiles[blk] = rows, ftile
            plan.dense_schemes[blk] = 'f16x2-image'
            w16 = plan._packed_weights(layer, 'f16x2', rows)
            part = partials()             # (both legs -- fp16 image, bf16x3 for extreme utterances -- write their utterances' partials)
            w3 = plan._packed_weights(layer, 'bf16x3')
            plan._timed('dense_conv', meta, lambda: hip.dense_conv1d_first_ranged(
                src, frames, rng, w16, w3, conv.out_channels, layer.kernel_size, bias, out, layer.strides, image, rows, part, ftile))
        elif self.image is not None:
            image, bound = self.image
            plan.dense_schemes[blk] = 'f16x2-image'
            b, c, ld = src.shape
            rows, ftile = tiles.dense_tile(plan.batch, conv.in_channels, conv.out_channels, layer.strides, (frames + layer.strides - 1) // layer.strides)
            plan.dense_row_tiles[blk], plan.dense_frame_tiles[blk] = rows, ftile
            part = partials()
            w16 = plan._packed_weights(layer, 'f16x2', rows)
            plan._timed('dense_conv', meta, lambda: hip.dense_conv1d_fused_packed_f16_img(
                image, bound, b, c, frames, ld, w16, conv.out_channels, layer.kernel_size, bias, out, layer.strides, rows, part, ftile))
        elif plan.dense_mode != 'f32' and layer.kernel_size == 8:
            scheme = 'f16x2' if plan.dense_mode == 'auto' and absmax is not None and ln is None else 'bf16x3'
            plan.dense_schemes[blk] = scheme
            part = partials()             # (the same 16-channel partials as the image path: the statistics do not depend on the route)
            packed = plan._packed_weights(layer, scheme)
            plan._timed('dense_conv', meta, lambda: hip.dense_conv1d_fused_packed(
                src, frames, packed, conv.out_channels, layer.kernel_size, bias, (), out, layer.strides, ln, scheme,
                absmax if scheme == 'f16x2' else None, part))
        else:
            plan.dense_schemes[blk] = 'f32'
            part = None
            plan._timed('dense_conv', meta, lambda: hip.dense_conv1d_fused(src, frames, conv.weight.detach(), bias, (), out,
                                                                          layer.strides, ln, ln is not None, False))
        return part

    def norm(self, idx, norm, nxt, after, partials):
        self.layernorm(idx, norm, nxt, cheap_consumer(nxt), partials)

    def after_cell(self, idx, norm, nxt, after, partials):
        if self.pipe and isinstance(nxt, (nn.Dropout, nn.LSTM)):
            self.tail_slot, _ = self.plan._pipeline_buffers(self.act.shape[1], self.frames, need_enc=False, group=self.group)
        if norm is None:
            return self.tap(idx)
        self.layernorm(idx, norm, nxt, self.defers(nxt, after), partials)

    def layernorm(self, idx, norm, nxt, defer, partials):
        """LayerNorm of `act`: left pending where the consumer normalises on load (``defer``), else in place -- together with what a
        dense convolution behind it needs (the split-fp16 operand image, or the range bound)."""
        plan, meta = self.plan, self.norm_meta()
        if defer:
            return self.defer_norm(idx, norm, meta, partials)
        act, frames, gamma, beta, eps = self.act, self.frames, norm.weight.detach(), norm.bias.detach(), norm.eps
        want_range = plan.dense_mode == 'auto' and isinstance(nxt, PadConvRelu) and nxt.groups == 1 and nxt.kernel_size == 8
        if want_range and self.taps is None:
            # the consumer is the fp16-split convolution: write its pre-split operand image instead of the fp32 tensor
            # (same traffic; the convolution then gathers its tiles by LDS-DMA and does no vector staging)
            b, c, ld = act.shape
            image = plan._buf('image', max(hip.load_library().nbasr_split_image_bytes(b, c, ld), 16), torch.uint8)
            stats, bound = self.next_stats(), plan.absmax[:b]
            plan._timed('layernorm', meta, lambda: hip.layernorm_split_image(act, gamma, beta, stats, bound, image, frames, eps))
            self.image = (image, bound)
            return
        absmax = plan.absmax[: act.shape[0]] if want_range else None
        plan._timed('layernorm', meta, lambda: hip.layernorm_channels(act, gamma, beta, act, frames, eps, absmax))
        self.absmax = absmax
        self.tap(idx)

    def project(self, layer, b_ih, b_hh, gates, meta):
        if self.plan.linear_mode == 'f16x2':
            return self.project_packed(layer, b_ih, b_hh, gates, meta)
        src, frames, ln, w_ih = self.act, self.frames, self.pending, layer.weight_ih_l0.detach()
        self.plan._timed('lstm_projection', meta, lambda: hip.lstm_input_projection(src, frames, w_ih, b_ih, b_hh, gates, layer.hidden_size, ln))

    def group_tail(self, idx, layer, b_ih, b_hh, meta):
        """TAIL GROUP (round 6): this forward's gates become utterances g * batch .. of the group's (frames, n * batch, 4 hidden) gate tensor; the
        last member runs ONE recurrence and ONE head over all of them -- a frame of the recurrence costs at 32 utterances what it costs at
        8, and no utterance's h depends on the batch it is computed in (bit-identical).  Returns the member's handle."""
        plan, frames, hidden = self.plan, self.frames, layer.hidden_size
        g, n = self.group
        gb = n * plan.batch
        gates_all = plan.gates_group[self.tail_slot]
        self.project_packed(layer, b_ih, b_hh, gates_all, meta, batch_total=gb, batch_offset=g * plan.batch)
        if g < n - 1:
            return plan._group_member(self.group, None)
        self.enter_tail()
        xcd_ws = plan._buf('lstm_xcd_group', hip.lstm_xcd_workspace_bytes(gb, hidden), torch.uint8)
        cell_all = plan._buf('cell_group', gb * hidden)[: gb * hidden]
        h_all = plan._buf('h_out_group', gb * frames * hidden)[: gb * frames * hidden].view(gb, frames, hidden)
        gview = gates_all[: frames * gb * 4 * hidden].view(frames, gb, 4 * hidden)
        plan._timed('lstm', meta, lambda: hip.lstm_recurrence_frames16(gview, plan._packed_whh16(layer.weight_hh_l0), cell_all, h_all, xcd_ws))
        head = self.layers[idx + 1]
        logits = plan._new_logits((gb, frames, head.out_features), torch.float32, True)
        hip.linear_head(h_all, head.weight.detach(), head.bias.detach(), logits)
        self.leave_tail()
        return plan._group_member(self.group, logits)

    def head(self, idx, layer):
        logits = self.plan._new_logits((self.plan.batch, self.frames, layer.out_features), torch.float32, self.tail_ctx is not None)
        self.head_into(layer, logits)
        self.act, self.pending, self.logits = logits, None, logits


class WalkBf16(Walk):
    """Activations and GEMM operands STORED as bfloat16 (what `model.to(torch.bfloat16)(x.bfloat16())` is in the reference): dense convs
    as one bf16 MFMA per product on a producer-written operand image, node ops / LayerNorm reading and writing bf16 rows (pitch: 8 frames,
    half the HBM bytes) with fp32 arithmetic and ONE rounding per tensor; LayerNorm statistics, LSTM gates / state and the head in fp32 --
    the kernels read fp32 copies of the parameters --; logits returned as bfloat16."""
    dtype = torch.bfloat16

    def __init__(self, plan, model, x, taps, pipelined, capturing, group=None):
        super().__init__(plan, model, x, taps, pipelined, capturing, group)
        self.copies = plan
        if x.shape[-1] % 8 or x.data_ptr() % 16:        # model input -> pitched bf16 rows (whole 16-byte chunks)
            self.cur = 2
            self.act = hip.repitch(x, plan._view(2, x.shape[1], plan.frames, self.dtype), plan.frames)

    def f32(self, param):
        return self.plan._f32(param)

    def gc_variant(self, view, node, ln0, stats, n_inputs):
        # 8 frames per lane (16-byte accesses) where rows are long; the narrow blocks run better as more, lighter waves
        # (tools/bench_gc_variants.py on an MI355X: 40 vs 49 us at 1 600 frames, 39 vs 37 us at 400)
        return (hip.GC_FPL8 | hip.GC_WPERM) if self.frames >= 512 else hip.GC_WPERM

    @staticmethod
    def defers(nxt, after):
        return cheap_consumer(nxt) or isinstance(after, nn.LSTM)

    def image_of(self, norm=None, stats=None, eps=0.0):
        """The dense convolution's operand image of `act` -- of its LayerNorm with ``norm`` = (gamma, beta), which also fills ``stats``."""
        b, c, ld = self.act.shape
        image = self.plan._buf('image16', max(hip.load_library().nbasr_bf16_image_bytes(b, c, ld), 16), torch.uint8)
        return hip.bf16_image(self.act, image, self.frames, norm, stats, eps)

    def dense_conv(self, idx, layer, out, t_out, meta):
        plan, conv, blk = self.plan, layer.conv, self.blk
        if self.pending is not None:
            raise RuntimeError('a dense convolution cannot take a deferred LayerNorm in the bf16 path')
        image = self.image if self.image is not None else self.image_of()
        rows, ftile = tiles.bf16_tile(plan.batch, conv.out_channels, t_out, self.pipe)
        plan.dense_row_tiles[blk], plan.dense_frame_tiles[blk] = rows, ftile
        w = conv.weight
        packed = plan._cached(w, ('bf16', rows, layer.strides), lambda: hip.pack_dense_weights_bf16(plan._f32(w), layer.strides, rows))
        bias, frames, (b, c, ld) = plan._f32(conv.bias), self.frames, self.act.shape
        plan.dense_schemes[blk] = 'bf16'
        plan._timed('dense_conv', meta, lambda: hip.dense_conv1d_bf16_img(image, b, c, frames, ld, packed, conv.out_channels, layer.kernel_size,
                                                                          bias, out, layer.strides, rows, ftile))
        return None

    def fused(self, layer, mask, out, want_stats):
        plan, nodes = self.plan, layer.nodes
        groups = nodes[-1].op.groups
        if not (plan.cell_mfma and hip.grouped_cell_mfma_fits(layer.filters, self.act.shape[2], groups)):
            return super().fused(layer, mask, out, want_stats)      # (x1 and x2 rounded to bf16 exactly where the node launches store them)
        # every tensor of the bf16 model is a bfloat16 tensor: the products go to the matrix cores unchanged (grouped_cell_mfma.hip;
        # 133 against 281 us for a 32 x 800 x 1600 cell).  That kernel has no statistics by-product: a consumer that
        # normalises on load gets them from a read pass over the result (~25 us)
        biases = [plan._f32(n.op.conv.bias) for n in nodes]
        specs = [(plan._cached(n.op.conv.weight, 'cell_mfma', lambda w=n.op.conv.weight: hip.grouped_cell_mfma_pack(plan._f32(w), groups)),
                  bias, n.op.kernel_size, n.op.dilation) for n, bias in zip(nodes, biases)]
        src, frames, ln0 = self.act, self.frames, self.pending
        plan._timed('grouped_cell_mfma', self.fused_meta(layer), lambda: hip.grouped_cell_mfma(src, specs, mask, out, frames, groups, ln0))
        return False

    def norm(self, idx, norm, nxt, after, partials):
        """What follows a cell (``norm``: its LayerNorm or None) or is a block LayerNorm: pending for a consumer that normalises on load
        (a grouped-conv cell, the LSTM's projection), as the operand image for a dense convolution, as fp32 rows for the head, else in place."""
        plan, act, frames, meta = self.plan, self.act, self.frames, self.norm_meta()
        feeds_tail = isinstance(nxt, (nn.Dropout, nn.LSTM, nn.Linear))
        if feeds_tail and isinstance(after, nn.LSTM):
            # the LSTM's input projection takes the bf16 encoder output itself (round 4: bf16 operand image, one MFMA per
            # product) and applies a pending LayerNorm while writing that image: statistics only, no fp32 copy of the tensor
            if self.pipe:
                self.tail_slot, _ = plan._pipeline_buffers(act.shape[1], act.shape[2], need_enc=False)
            if norm is not None:
                return self.defer_norm(idx, norm, meta, partials)
        elif feeds_tail:
            # hand-over to the fp32 tail (the head): the last LayerNorm writes fp32
            b, c, ld = act.shape
            if self.pipe:
                self.tail_slot, enc = plan._pipeline_buffers(c, ld)           # fp32 (B, C, ld) double buffer
            else:
                enc = plan._buf('enc32', b * c * ld)[: b * c * ld].view(b, c, ld)
            if norm is not None:
                gamma, beta, eps = plan._f32(norm.weight), plan._f32(norm.bias), norm.eps
                plan._timed('layernorm', meta, lambda: hip.layernorm_channels(act, gamma, beta, enc, frames, eps))
            else:
                hip.convert(act, enc)
            self.act, self.cur = enc, None
        elif norm is not None:
            if cheap_consumer(nxt):
                return self.defer_norm(idx, norm, meta, partials)
            gamma, beta, eps = plan._f32(norm.weight), plan._f32(norm.bias), norm.eps
            stats = self.next_stats()
            if isinstance(nxt, PadConvRelu):
                # the consumer is a dense conv: the LayerNorm writes its operand image (statistics on the way)
                self.image = plan._timed('layernorm', meta, lambda: self.image_of((gamma, beta), stats, eps))
                return self.tap_normalised(idx, gamma, beta, eps)
            plan._timed('layernorm', meta, lambda: hip.layernorm_channels(act, gamma, beta, act, frames, eps))
        self.tap(idx)

    after_cell = norm

    def project(self, layer, b_ih, b_hh, gates, meta):
        plan = self.plan
        for w in (layer.weight_ih_l0, layer.weight_hh_l0):
            plan._f32(w)              # both fp32 copies are made here, on the main stream, before the tail moves to the side stream
        if self.act.dtype == torch.float32:
            # (an fp32 hand-over copy of the encoder output, should a caller's layer list have made one: the fp16-split GEMM of rounds 2-3)
            return self.project_packed(layer, b_ih, b_hh, gates, meta)
        src, frames = self.act, self.frames
        packed_ih, ws = plan._packed_linear_bf16(layer.weight_ih_l0), plan._pointwise_bf16_ws(*src.shape)
        ln, self.pending = self.pending, None
        plan._timed('lstm_projection', meta, lambda: hip.lstm_input_projection_bf16(src, frames, packed_ih, b_ih, b_hh, gates, layer.hidden_size, ws, ln))

    def head(self, idx, layer):
        plan, (rows, cols, classes) = self.plan, (self.plan.batch, self.frames, layer.out_features)
        n = rows * cols * classes
        n8 = max((n + 7) & ~7, 8)
        logits32 = plan._buf('logits32', n8)[:n8]       # tails run one after another on the side stream
        self.head_into(layer, logits32[:n].view(rows, cols, classes))
        # (the conversion works in 8-element chunks: the last chunk's padding is converted too and never returned)
        out16 = plan._new_logits((rows, cols, classes), self.dtype, self.tail_ctx is not None, numel=n8)
        hip.convert(logits32, out16)
        self.act = self.logits = out16[:n].view(rows, cols, classes)


def run(plan, model, x, taps, pipelined, capturing, group=None):
    """Enqueue one forward of ``model`` through ``plan``: the body of ``ForwardPlan._enqueue``, what a launch tape records."""
    walk = WalkBf16 if x.dtype == torch.bfloat16 else WalkF32
    return walk(plan, model, x, taps, pipelined, capturing, group).run()
