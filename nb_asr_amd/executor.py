"""Host-side executor: the plan behind the walk over the model's layer list that enqueues the HIP kernels.

Replaces the isinstance-dispatch loop of the reference's ``ASRModel.forward`` (model.py:116-131),
``SearchCell.forward`` (model.py:49-59) and ``Node.forward`` (model.py:13-22):

* activations stay in (batch, channels, frames) order in pitched workspace buffers (row pitch =
  frames rounded up to 4, pitch columns kept at zero), so none of the reference's permutes, padded
  copies, ``zeros_like`` branches or ``0 + x`` adds exist here;
* a node is ONE launch: main op + bias + ReLU + clamp + the sum of its flagged skip inputs;
* LayerNorm runs on the channel (slow) dimension in place.

Four workspace buffers sized for the widest block are rotated; nothing is allocated per call
except the returned logits.  A plan belongs to a DEVICE, not to a (batch, frames) shape and not to a model
object: its workspaces only ever grow (a stream of TIMIT batches whose length differs every step re-uses the
same memory), and the model is passed to every call, so ``torch.nn.DataParallel`` replicas (shallow copies of
the module that share the plan pool) each run with their own parameters.

This module keeps what outlives a call: ``ForwardPlan`` (workspaces, derived-weight cache, the LSTM recurrence, captured graphs, the
pipelined tail's streams and buffers) and ``PlanPool``.  What a plan merely uses has a module of its own: the tile and kernel-variant
choices are the free functions of ``tiles.py``; launch tapes -- key, record-or-replay, the one ``invalidate()`` -- are ``tape.py``; the
ring of recurrence status words is ``seq_status.py``.  The launch sequence of ONE forward -- a dispatch loop over ``model.model`` with
one step per layer kind, shared by the fp32 and the bf16 storage path, and the state that forward carries -- is ``walk.py``;
``node_into`` below is the one node launch both of them (and ``Node.forward``, ``streaming``) go through.
"""
import os
import threading
import weakref

import torch

from . import hip, seq_status, tape
from .tape import LaunchTape, _structure_epoch          # noqa: F401  (tests build a LaunchTape and read the epoch through this module)


def node_into(node, inputs, frames, out, ln0=None, stats=None, linear_ctx=None, gc_variant=0, copies=None):
    """Enqueue one cell node: ``out = op(inputs[-1]) + sum(flagged inputs)`` (left-to-right).

    ``ln0`` = (stats, gamma, beta): ``inputs[0]`` (the cell input) is stored un-normalised with a pending LayerNorm that
    the kernel applies while loading -- as the main input when the node is the cell's first, as skip0 when flagged.
    ``stats`` = (stats_out, workspace, eps): a grouped-conv node also emits the LayerNorm statistics of ``out``.
    ``linear_ctx`` = (packed_weights(op), workspace(c_in, ld)) callables of a ForwardPlan: `linear` ops then run on the fp16
    matrix cores (packed weights, pre-split activations); None = the exact-fp32 MFMA GEMM.
    ``copies``: the ForwardPlan of a forward on bf16 rows.  Its parameters are bfloat16 tensors while the kernels read fp32 weights, so
    they come from the plan's derived copies: fp32 values, the [group][ci][tap][co] order for a GC_WPERM variant, the one-term bf16
    operand image of a `linear` op (one bf16 MFMA per product, gemm_pointwise.hip)."""
    from .ops import PadConvRelu, Linear, Zero, Identity
    f32 = copies._f32 if copies is not None else torch.Tensor.detach
    if len(inputs) != len(node.branch_ops):
        raise AssertionError('Branch op and input list have different lenghts')
    skips = [src for branch, src in zip(node.branch_ops, inputs) if isinstance(branch, Identity)]
    op, last = node.op, inputs[-1]
    on_x = ln0 is not None and len(inputs) == 1
    on_s0 = ln0 is not None and isinstance(node.branch_ops[0], Identity)       # the cell input, if flagged, is skips[0]
    ln = ln0 if (on_x or on_s0) else None
    if isinstance(op, PadConvRelu):
        # with `stats` the epilogue writes partial statistics to the workspace; the caller merges them (finalize)
        weight = copies._packed_grouped(op) if copies is not None and gc_variant & hip.GC_WPERM else f32(op.conv.weight)
        hip.grouped_conv1d_node(last, weight, f32(op.conv.bias), skips, out, frames,
                                op.groups, op.kernel_size, op.dilation, ln, on_x, on_s0,
                                stats[1] if stats is not None else None, gc_variant)
    elif isinstance(op, Linear):
        if stats is not None:
            raise ValueError('statistics from the epilogue are only available for grouped-conv nodes')
        if copies is not None:
            packed, ws = copies._packed_linear_bf16(op.linear.weight), copies._pointwise_bf16_ws(*last.shape)
            hip.linear_fused_bf16(last, frames, packed, op.linear.out_features, f32(op.linear.bias), skips, out, ws, ln, on_x, on_s0)
        elif linear_ctx is not None:
            packed, workspace = linear_ctx
            hip.linear_fused_packed(last, frames, packed(op.linear), op.linear.out_features, op.linear.bias.detach(), skips, out,
                                    workspace(last.shape[1], last.shape[2]), ln, on_x, on_s0)
        else:
            hip.dense_conv1d_fused(last, frames, op.linear.weight.detach().unsqueeze(-1), op.linear.bias.detach(),
                                   skips, out, 1, ln, on_x, on_s0)
    elif isinstance(op, Zero):
        hip.skip_sum(skips, out, frames, ln if on_s0 else None, on_s0)
    else:
        raise TypeError(f'unsupported node operation {type(op).__name__}')
    return out


class PendingLogits:
    """Logits produced on the plan's side stream (pipelined forward).  ``result()`` makes the caller's current stream
    wait for them -- until then the next batch's encoder may already be running on the main stream."""

    def __init__(self, logits, event):
        self._logits, self._event = logits, event
        self._seq = None             # (plan, event behind the status copy, ring slot) when this forward ran the one-launch recurrence

    def result(self):
        """The logits, ordered behind the tail on the caller's current stream (no host wait) -- except for a forward whose LSTM
        recurrence ran as ONE resident launch (NBASR_LSTM_SEQ=1 in pipelined mode): that launch can time out when another process
        takes its compute units, so ``result()`` then waits for ITS status word and raises ``HipError`` instead of handing out the
        NaN rows.  A plain ``model(x)`` returns a tensor, not a handle: it can only report at the next call or
        through ``model.check()``."""
        if self._event is not None:
            cur = torch.cuda.current_stream(self._logits.device)
            cur.wait_event(self._event)
            self._logits.record_stream(cur)
            self._event = None
        if self._seq is not None:
            (plan, ev, slot), self._seq = self._seq, None
            plan.check_seq_slot(ev, slot)
        return self._logits


class GroupLogits(PendingLogits):
    """Handle of a pipelined forward whose LSTM + head run together with those of the other forwards of its TAIL GROUP (round 6,
    `ASRModel.forward_many(tail_group=...)`): the logits exist once the group's last forward has been enqueued."""

    def __init__(self):
        super().__init__(None, None)

    def _set(self, logits, event):
        self._logits, self._event = logits, event

    def result(self):
        if self._logits is None:
            raise hip.HipError('this forward belongs to a tail group whose last forward has not been enqueued yet '
                               '(forward_many enqueues a whole group before it reads a result)')
        return super().result()


# Environment switches of earlier rounds that no longer exist: a script that still sets one gets ONE warning instead of silence
_REMOVED_SWITCHES = {
    'NBASR_TRAIN_GEMM': 'folded into NBASR_DENSE_MODE (f32 = every GEMM on the exact-fp32 MFMA)',
    'NBASR_IMAGE_MODE': None, 'NBASR_ROW_TILE': None, 'NBASR_LN_MODE': None, 'NBASR_EPILOGUE_STATS': None, 'NBASR_LSTM_UNPACKED': None,
    'NBASR_GC_TABLE': 'NBASR_GC_F32_VARIANT=0 runs the default node kernel everywhere', 'NBASR_GC_BF16_VARIANT': None,
    'NBASR_GC_BF16_MFMA': 'NBASR_CELL_FUSION=1|valu|0 chooses the bf16 cell kernel', 'NBASR_MFMA_SPLITS': None,
    'NBASR_DENSE_EPILOGUE': None, 'NBASR_FORCE_DIST': None, 'NBASR_PW_ORDER': None,
}
_warned_removed = [False]


def _warn_removed_switches():
    if _warned_removed[0]:
        return
    _warned_removed[0] = True
    stale = [k for k in _REMOVED_SWITCHES if k in os.environ]
    if stale:
        import warnings
        notes = '; '.join(f'{k} ({_REMOVED_SWITCHES[k]})' if _REMOVED_SWITCHES[k] else k for k in stale)
        warnings.warn(f'nb_asr_amd: these environment switches were removed and are IGNORED: {notes}.  The current ones: NBASR_DENSE_MODE, '
                      f'NBASR_LINEAR_MODE, NBASR_CELL_FUSION, NBASR_GC_F32_VARIANT, NBASR_LSTM_SEQ, NBASR_TAPE, NBASR_CONV_STATS (DESIGN.md 5)', stacklevel=3)


class ForwardPlan:
    """Workspaces + launch sequence for one device.  Shape-independent: every buffer is flat, grows on demand
    (never shrinks) and is viewed per call; at most one forward is being ENQUEUED through a plan at a time
    (``PlanPool`` hands a plan to one thread at a time), while pipelined tails of earlier calls may still be in flight."""

    def __init__(self, device):
        _warn_removed_switches()
        self.device = torch.device(device)
        self.batch = self.frames = self.out_frames = 0
        self.block_frames = []
        self.timer = None
        self.dense_mode = hip.dense_mode()        # dense k=8 convs: 'auto' | 'bf16x3' | 'f32', all fp32-accurate (what each means: there)
        self._packed = {}            # (id(parameter), tag) -> (weakref(parameter), version, packed tensor)
        # per-frame linear maps (`linear` node ops, LSTM input projection): 'f16x2' = fp16 matrix cores with pre-split
        # activations (default), 'f32' = the exact-fp32 MFMA GEMM
        self.linear_mode = os.environ.get('NBASR_LINEAR_MODE', 'f16x2')
        if self.linear_mode not in ('f16x2', 'f32'):
            raise ValueError(f'NBASR_LINEAR_MODE must be f16x2 or f32, got {self.linear_mode!r}')
        self.dense_schemes = {}      # block -> scheme used by the last run (read by bench.py)
        self.dense_row_tiles = {}    # block -> rows per workgroup of the image-path GEMM in the last run
        self.dense_frame_tiles = {}  # block -> frames per workgroup (256, or 128 where the measured table says so)
        # cells whose three nodes are grouped convs run as ONE launch where a row fits a workgroup (<= 1024 frames): x1 and x2 never
        # touch HBM and the cell's LayerNorm statistics come out of the same launch (grouped_cell.hip, round 3).  Bit-identical to
        # the three node launches; NBASR_CELL_FUSION=0 turns it off (A/B)
        _cf = os.environ.get('NBASR_CELL_FUSION', '1')
        if _cf not in ('1', '0', 'valu'):
            raise ValueError(f"NBASR_CELL_FUSION={_cf!r}: expected '1', '0' or 'valu'")
        self.cell_fusion = _cf != '0'
        self.cell_mfma = _cf == '1'          # bf16 storage: the matrix-core cell kernel ('valu': the vector-ALU one, as for fp32)
        # the LSTM recurrence (round 6: fp16-pair matrix cores, a tile of 16 utterances per workgroup row): 'auto' = ONE resident launch whose
        # exchange stays inside an XCD (nbasr_lstm_recurrence_xcd) in the plain forward and in a captured graph, the same arithmetic as one
        # launch per frame (nbasr_lstm_recurrence_frames16) in a pipelined tail on the side stream; 'xcd' / 'frames' = that form everywhere
        # ('frames' is also what a failed status word demotes a plan to); the fp32-MFMA kernels of rounds 1-5, another summation order:
        # '0' = one launch per frame, '1' = the chip-wide resident grid (bit-identical to '0') wherever it applies
        self.lstm_seq_mode = os.environ.get('NBASR_LSTM_SEQ', 'auto')
        if self.lstm_seq_mode not in ('auto', 'xcd', 'frames', '0', '1'):
            raise ValueError(f"NBASR_LSTM_SEQ={self.lstm_seq_mode!r}: expected 'auto', 'xcd', 'frames', '0' or '1'")
        self.tail_mode = os.environ.get('NBASR_TAIL', 'auto')
        if self.tail_mode not in ('auto', 'side', 'main'):
            raise ValueError(f"NBASR_TAIL={self.tail_mode!r}: expected 'auto', 'side' or 'main'")
        self._group_handles = []      # handles of the tail group being enqueued (_group_member)
        self._released_on, self._released_event = None, None   # PlanPool: the stream the last forward was enqueued on, an event behind it
        self.seq_status = seq_status.SeqStatusRing()     # the status words of the one-launch recurrences (check_seq, check_seq_slot)
        self._seq_last = None        # (event, slot) of the status copy the forward being enqueued has just added
        # statistics of a downsample convolution's output from its own epilogue (round 5); NBASR_CONV_STATS=0: a pass over the output
        self.conv_stats = os.environ.get('NBASR_CONV_STATS', '1') != '0'
        self._seq_flags = hip.LSTM_SEQ_INJECT_FAULT if os.environ.get('NBASR_LSTM_SEQ_FAULT') == '1' else 0     # tests: force a timeout
        self._bufs = {}              # name -> flat tensor; grow-only (see _buf)
        self.grow_count = 0          # number of (re)allocations so far (tests: a smaller batch must not allocate)
        # pipelined mode (forward_async): the latency-bound LSTM + head of batch i run on a side stream while the main
        # stream already runs the encoder of batch i+1; the encoder output is double-buffered for that
        self.side_stream = None
        self._graphs = {}            # (batch, frames) -> (graph, parameter signature, x_static, y_static)
        self.tail_done = [None, None]
        self._turn = 0
        # launch tapes (tape.py): NBASR_TAPE=0 issues every forward through the python launch sequence
        self.tape_mode = os.environ.get('NBASR_TAPE', '1') != '0'
        self.tapes = tape.Tapes()            # (tests read and set its state through _tapes, tape_replays and _recording below)
        self._tape_logits = None     # the logits of the forward being enqueued (_new_logits): what a replay hands out

    _tapes = property(lambda self: self.tapes.tapes)
    tape_replays = property(lambda self: self.tapes.replays)
    _recording = property(lambda self: self.tapes.recording, lambda self, entries: setattr(self.tapes, 'recording', entries))

    # ---- grow-only workspaces ---------------------------------------------------------------------------------------
    def _buf(self, name, numel, dtype=torch.float32):
        """Flat workspace ``name`` with at least ``numel`` elements.  Growing re-allocates: pipelined tails that may
        still read the old memory are waited for first (stream-ordered, no host sync), and captured graphs die."""
        t = self._bufs.get(name)
        if t is None or t.numel() < numel or t.dtype != dtype:
            self.wait_tails()
            self._graphs.clear()
            self.tapes.invalidate()
            t = self._bufs[name] = torch.empty(max(int(numel), 4), device=self.device, dtype=dtype)
            if self.side_stream is not None:
                t.record_stream(self.side_stream)
            self.grow_count += 1
        return t

    def _recurrence(self, gates, w_hh, hidden, pipe, capturing=False):
        """The LSTM recurrence into ``self.h_out``.  Round 6: ONE resident launch with a tile of 16 utterances per XCD on the fp16 matrix
        cores (nbasr_lstm_recurrence_xcd) wherever it applies -- plain forward, pipelined tail and captured graph alike (every route the same
        arithmetic); a layer wider than 512 or a plan demoted by a failed status word takes one launch per frame (replayed as a graph)."""
        # (launches of the resident grid are chained across the process's streams by an event, which a graph capture cannot hold)
        if not capturing and torch.cuda.is_current_stream_capturing():       # a caller's own torch.cuda.graph(...) around model(x)
            capturing = True
        mode = self.lstm_seq_mode
        # 'auto': the resident launch everywhere except in a tail on the SIDE stream -- a resident grid there fills whole XCDs (32 compute
        # units each, for the length of the recurrence) while the hardware deals every workgroup of the next batch's encoder kernels to a
        # fixed XCD: the encoder stalls on the occupied ones (measured, round 6: 9 620 against 9 995 utterances/s at 64, 4 136 against
        # 5 398 at 8).  There, and in a plan demoted by a failed status word ('frames'), the SAME arithmetic runs as one launch per frame
        # (nbasr_lstm_recurrence_frames16): every route of the default configuration gives the same bits
        if mode in ('auto', 'xcd', 'frames'):
            nbytes = hip.lstm_xcd_workspace_bytes(self.batch, hidden)
            if nbytes:
                ws = self._buf('lstm_xcd', nbytes, torch.uint8)
                if mode == 'xcd' or (mode == 'auto' and not pipe):
                    out = hip.lstm_recurrence_xcd(gates, self._packed_whh16(w_hh), self.cell_ws, self.h_out, ws, self._seq_flags)
                    if not capturing:          # (a captured graph holds the launch, not the host-side read-back of its status word)
                        self._host(lambda: self._seq_launched(ws))
                    return out
                return hip.lstm_recurrence_frames16(gates, self._packed_whh16(w_hh), self.cell_ws, self.h_out, ws)
        packed_hh = self._packed_whh(w_hh)
        nbytes = hip.lstm_seq_workspace_bytes(self.batch, hidden, self.device) if (mode == '1' and not capturing) else 0
        if nbytes:
            ws = self._buf('lstm_seq', nbytes, torch.uint8)
            try:
                out = hip.lstm_recurrence_seq(gates, packed_hh, self.cell_ws, self.h_out, ws, self._seq_flags)
            except hip.HipError as e:
                # ONLY the device refusing the cooperative grid (a partition / CU mask smaller than the occupancy query said) demotes the
                # plan to per-frame launches; an argument, alignment or capture error is the caller's to see.  The refusal is
                # recognised by its CODE (hipErrorCooperativeLaunchTooLarge, passed through by the entry point), not by its wording
                if e.code != hip.HIP_ERROR_COOPERATIVE_LAUNCH_TOO_LARGE:
                    raise
                self.lstm_seq_mode = '0'
                self.tapes.invalidate()       # a tape being recorded right now holds the refused launch: it must not be kept
                return hip.lstm_recurrence_packed(gates, packed_hh, self.cell_ws, self.h_out)
            self._host(lambda: self._seq_launched(ws))
            return out
        return hip.lstm_recurrence_packed(gates, packed_hh, self.cell_ws, self.h_out)

    def _seq_launched(self, ws):
        """Host step behind every one-launch recurrence (recorded into a tape with it): its status word sets out for the ring."""
        self._seq_last = self.seq_status.launched(ws, self.device)

    def _demote(self):
        """After a resident recurrence reported a timeout: one launch per frame from now on, in the SAME arithmetic as the form that failed.
        May run on the thread that reads a result while another one records a tape through this plan: that tape holds the resident launch
        and the tape key does not hold ``lstm_seq_mode``, so it must not be kept either."""
        self.lstm_seq_mode = '0' if self.lstm_seq_mode == '1' else 'frames'
        self.tapes.invalidate()

    def seq_pending(self):
        """Whether a one-launch recurrence enqueued through this plan still awaits a look at its status word."""
        return bool(self.seq_status.pending)

    def check_seq(self, wait=False):
        """Raise if a one-launch recurrence enqueued through this plan timed out (that forward's logits hold NaN rows); the
        one-launch form is switched off for this plan then, so the caller's retry runs the per-frame launches.  ``wait``: block until
        that launch has finished (tests, `ASRModel.check`); otherwise only a finished launch is looked at -- called at the start of
        every forward, so a failure surfaces at the next call at the latest."""
        if self.seq_status.poll(wait):
            self._demote()
            raise hip.HipError('the one-launch LSTM recurrence of an EARLIER forward timed out waiting for its peer workgroups (the grid was '
                               'not co-resident: compute units taken by another process or stream); that forward\'s logits are invalid. '
                               'The plan now uses one launch per frame (same arithmetic): run the forward again')

    def check_seq_slot(self, ev, slot):
        """Wait for ONE one-launch recurrence (the status copy behind it) and raise if it timed out: what ``PendingLogits.result()``
        does for the forward it belongs to."""
        if self.seq_status.verdict(ev, slot):
            self._demote()
            raise hip.HipError('the one-launch LSTM recurrence of THIS forward timed out waiting for its peer workgroups (the grid was not '
                               'co-resident: compute units taken by another process or stream); its logits are invalid. The plan now '
                               'uses one launch per frame (as NBASR_LSTM_SEQ=0): run the forward again')

    def wait_tails(self):
        """Make the current stream wait for every pipelined LSTM tail enqueued through this plan (a plain
        forward after forward_async shares the gate / cell / h buffers with the tail that is still running)."""
        cur = None
        for k, ev in enumerate(self.tail_done):
            if ev is not None:
                cur = cur or torch.cuda.current_stream(self.device)
                cur.wait_event(ev)

    def close(self):
        """Called before the plan is dropped: later allocations on the current stream may re-use its memory."""
        self.wait_tails()
        self._graphs.clear()
        self.tapes.invalidate()
        self._bufs.clear()
        self.side_stream = None                     # (streams.py remembers it for the main stream: a plan built again gets the same one)

    def _set_shape(self, batch, frames, use_rnn, dtype=torch.float32):
        from .model import FILTERS, DOWN_STRIDES, LSTM_HIDDEN
        self.batch, self.frames = batch, frames
        t, self.block_frames = frames, []
        for s in DOWN_STRIDES:
            t = (t + s - 1) // s
            self.block_frames.append(t)
        self.out_frames = self.block_frames[-1]
        pitch8 = lambda t: (t + 7) & ~7                  # noqa: E731  (bf16 rows are pitched to 8 frames: size for either storage type)
        stat_elems = max(batch * 2 * pitch8(t) for t in self.block_frames)
        self.stats = [self._buf(f'stats{i}', stat_elems) for i in range(2)]
        ws_bytes = hip.load_library().nbasr_grouped_stats_workspace_bytes(max(batch, 1), max(max(pitch8(t) for t in self.block_frames), 8), 100)
        self.stats_ws = self._buf('stats_ws', ws_bytes // 4)
        elems = max(batch * c * hip.round_up4(t) for c, t in zip(FILTERS, self.block_frames))
        self.pool = [self._buf(f'pool{i}', elems) for i in range(4)]
        self.absmax = self._buf('absmax', max(batch, 1))          # max|LayerNorm output| per utterance
        self.absmax_in = self._buf('absmax_in', max(batch, 1))    # max|model input| per utterance
        if use_rnn:
            self.gates_ws = self._buf('gates0', batch * self.out_frames * 4 * LSTM_HIDDEN)
            self.cell_ws = self._buf('cell', batch * LSTM_HIDDEN)
            self.h_out = self._buf('h_out', batch * self.out_frames * LSTM_HIDDEN)[: batch * self.out_frames * LSTM_HIDDEN] \
                .view(batch, self.out_frames, LSTM_HIDDEN)
        else:
            self.h_out = None
        if dtype == torch.bfloat16:                      # activations stored as bf16 rows, pitched to 8 frames
            elems = max(batch * c * hip.row_pitch(t, dtype) for c, t in zip(FILTERS, self.block_frames))
            self.pool16 = [self._buf(f'pool16_{i}', elems, dtype) for i in range(4)]

    def _timed(self, kind, meta, launch):
        """Run ``launch()``; when ``self.timer`` is a list, bracket it with HIP events on the current stream
        (bench.py's per-kernel roofline leg) and append (kind, meta, start, stop)."""
        if self.timer is None:
            return launch()
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        out = launch()
        stop.record()
        self.timer.append((kind, meta, start, stop))
        return out

    def _cached(self, param, tag, build):
        """Derived copy of a parameter (packed / split / re-laid-out), rebuilt whenever the parameter changes.  An entry is
        valid only for the very tensor OBJECT it was built from (weak reference) at the same version: a DataParallel
        replica's freshly broadcast weight may land at the address a dead one had, with the same version counter."""
        key = (id(param), tag)
        hit = self._packed.get(key)
        if hit is None or hit[0]() is not param or hit[1] != param._version:
            if len(self._packed) >= 512:
                self._packed = {k: v for k, v in self._packed.items() if v[0]() is not None}
            if hit is not None:
                self.wait_tails()        # a pipelined tail on the side stream may still read the copy that is being replaced
            built = build()
            if self.side_stream is not None and isinstance(built, torch.Tensor):
                built.record_stream(self.side_stream)
            hit = (weakref.ref(param), param._version, built)
            self._packed[key] = hit
            self.tapes.invalidate()
        return hit[2]

    def _packed_weights(self, layer, scheme, row_tile=128):
        """Split/re-laid-out copy of a downsample conv's weights."""
        w = layer.conv.weight
        return self._cached(w, (scheme, row_tile, layer.strides), lambda: hip.pack_dense_weights(w.detach(), layer.strides, scheme, row_tile))

    def _packed_linear(self, linear):
        """Packed (fp16 split) copy of an nn.Linear-like weight (c_out, c_in), rebuilt whenever the parameter changes."""
        w = linear.weight if hasattr(linear, 'weight') else linear
        return self._cached(w, 'pointwise', lambda: hip.pack_pointwise_weights(self._f32(w)))

    def _packed_linear_bf16(self, w):
        """One-term bf16 operand image of a per-frame linear map's (c_out, c_in) weight (bf16 storage), rebuilt whenever the parameter changes."""
        return self._cached(w, 'pointwise_bf16', lambda: hip.pack_pointwise_weights_bf16(self._f32(w)))

    def _packed_grouped(self, op):
        """[group][ci][tap][co] copy of a grouped conv's weights (what the fused cell's scalar loads read), rebuilt whenever the parameter changes."""
        w = op.conv.weight
        return self._cached(w, 'gc_wperm', lambda: hip.pack_grouped_weights(self._f32(w).contiguous(), op.groups))

    def _tail_on_side_stream(self, batch):
        """Where a pipelined forward (``forward_async``) runs its LSTM + head.  'side': on the plan's second stream, one launch per frame,
        beside the next batch's encoder (rounds 2-5).  'main': behind the encoder on the same stream, the recurrence as the resident
        XCD-local launch -- no overlap, but a recurrence of ~0.45 ms instead of 250 launches that take ~0.6 ms from the encoder they hide
        behind.  NBASR_TAIL=auto picks by batch size (measured table in DESIGN 6)."""
        if self.tail_mode == 'auto':
            return batch < self._TAIL_MAIN_FROM or self.lstm_seq_mode in ('0', '1')
        return self.tail_mode == 'side'

    _TAIL_MAIN_FROM = 1 << 30            # utterances per forward from which 'auto' keeps the tail on the main stream (set from measurements)

    def _packed_whh16(self, w):
        """w_hh as the resident operand image of the XCD-local recurrence (two fp16 terms per weight), rebuilt when the parameter changes."""
        return self._cached(w, 'whh16', lambda: hip.lstm_pack_whh16(self._f32(w).contiguous()))

    def _packed_whh(self, w):
        """Fragment-ordered copy of the LSTM's recurrent weight, rebuilt whenever the parameter changes."""
        return self._cached(w, 'whh', lambda: hip.lstm_pack_whh(self._f32(w).contiguous()))

    def _pointwise_ws(self, c_in, ld):
        need = hip.load_library().nbasr_pointwise_workspace_bytes(self.batch, c_in, ld)
        return self._buf('pointwise_ws', max(need, 16), torch.uint8)

    def _pointwise_bf16_ws(self, batch, c_in, ld):
        return self._buf('pointwise_bf16_ws', max(hip.load_library().nbasr_pointwise_bf16_workspace_bytes(batch, c_in, ld), 16), torch.uint8)

    def _dense_part(self, c_out, ld_out):
        """Workspace for the statistics partials a dense convolution emits from its epilogue (one row pair per 16 channels)."""
        n = hip.dense_stats_part_floats(self.batch, c_out, ld_out)
        return self._buf('dense_part', n)[:n]

    def _view(self, idx, channels, frames, dtype=torch.float32):
        ld = hip.row_pitch(frames, dtype)
        pool = self.pool16 if dtype == torch.bfloat16 else self.pool
        return pool[idx][: self.batch * channels * ld].view(self.batch, channels, ld)

    # ---- whole-forward HIP graph ------------------------------------------------------------------------------------
    def _signature(self, model):
        return tuple((p.data_ptr(), p._version) for p in model.parameters())

    def run_graph(self, model, x):
        """Replay the forward as ONE captured HIP graph (all ~350 launches incl. the 250 LSTM steps): removes the per-launch
        host cost and shortens the gaps between the short dependent kernels.  One graph per (batch, frames); re-captured
        when a parameter changes or a workspace grows.  Returns a tensor that the next run_graph call on the same shape
        overwrites."""
        sig = self._signature(model)
        key = (x.shape[0], x.shape[2])
        self.wait_tails()                                     # outside the capture: events of earlier pipelined calls
        hit = self._graphs.get(key)
        if hit is None or hit[1] != sig:
            self._graphs.pop(key, None)
            x_static = torch.empty(x.shape[0], x.shape[1], x.shape[2], device=self.device, dtype=x.dtype)
            x_static.copy_(x)
            for _ in range(2):                                # static initialisers, packed weights, workspace growth
                self.run(model, x_static)
            torch.cuda.synchronize(self.device)
            self.check_seq(wait=True)                         # (the warm-up forwards may have run the one-launch recurrence; the capture never does)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                y_static = self.run(model, x_static, _capturing=True)
            hit = self._graphs[key] = (graph, sig, x_static, y_static)
        hit[2].copy_(x)
        hit[0].replay()
        return hit[3]

    def _ensure_pipeline(self):
        if self.side_stream is not None:
            return
        # The tail's stream must sit on another hardware queue than the stream the encoder runs on -- and than every other stream this
        # package runs chains or tails on (two chains in flight: ASRModel.forward_many) -- or the overlap silently disappears: streams.py
        # probes pool streams for that.  Normal priority (round 6; rounds 1-5: high priority, "dispatched ahead of the encoder's bulk
        # work"): measured no gain from the priority (10 528 vs 10 548 utterances/s at 64 x 1000), and a high-priority queue starves the
        # normal-priority queue it shares a pipe with -- another chain's encoder, with two chains in flight.
        # (Measured and rejected: giving the tail 8-32 compute units of its own through CU-masked streams.  The 128
        # workgroups of a step then run in several rounds and the whole pipeline slows 2-3x; tools/ubench/cu_mask_map.hip
        # documents the mask layout.)
        from . import streams
        # (a chain stream of forward_many finds its tail stream chosen already; a lone caller's first pipelined forward probes here, waiting
        # for its own stream only when it runs beside other threads of the process)
        self.side_stream = streams.tail_stream_for(self.device, torch.cuda.current_stream(self.device), whole_device=threading.active_count() == 1)
        for t in self._bufs.values():                 # allocated on the main stream, from now on also read on the side stream
            t.record_stream(self.side_stream)
        for _, _, built in self._packed.values():     # derived weights (packed w_ih / w_hh, fp32 copies): read by the tails too
            if isinstance(built, torch.Tensor):
                built.record_stream(self.side_stream)

    def _pipeline_buffers(self, channels, frames, need_enc=True, group=None):
        """Double-buffered gate pre-activations of the pipelined tail (+ an fp32 hand-over copy of the encoder output where the
        storage types differ, bf16 path): (slot, encoder output view or None)."""
        from .model import LSTM_HIDDEN
        self._ensure_pipeline()
        ld = hip.round_up4(frames)
        enc = [self._buf(f'enc_out{i}', self.batch * channels * ld) for i in range(2)] if need_enc else None
        self.gates_pipe = [self.gates_ws, self._buf('gates1', self.batch * self.out_frames * 4 * LSTM_HIDDEN)]
        if group is not None:
            # a tail group: the gates of its n forwards in ONE (frames, n * batch, 4 hidden) tensor per slot; the slot turns with the
            # group's first forward, the others write into the slot that is current
            n_floats = group[1] * self.batch * self.out_frames * 4 * LSTM_HIDDEN
            self.gates_group = [self._buf('gates_group0', n_floats), self._buf('gates_group1', n_floats)]
            if group[0] > 0:
                return self._turn, None

        def rotate():
            self._turn ^= 1
            ev = self.tail_done[self._turn]
            if ev is not None:                       # the LSTM that read these buffers two forwards ago
                torch.cuda.current_stream(self.device).wait_event(ev)
        self._host(rotate)
        k = self._turn
        return k, (enc[k][: self.batch * channels * ld].view(self.batch, channels, ld) if need_enc else None)

    # ---- launch tapes ------------------------------------------------------------------------------------------------------
    def _host(self, step, produces=False):
        """Run a host-side step of the launch sequence now and, while a tape is being recorded, note it for every replay.
        ``produces``: the step returns a freshly allocated tensor whose address later launches take (patched on replay)."""
        out = step()
        recording = self.tapes.recording
        if recording is not None:
            recording.append([None, step, out.data_ptr() if produces else None, []])
        return out

    def _to_side_stream(self):
        """The launches that follow wait for everything enqueued on the current stream so far (host step of the tape)."""
        def hand_over():
            ready = torch.cuda.Event()
            ready.record(torch.cuda.current_stream(self.device))
            self.side_stream.wait_event(ready)
        self._host(hand_over)

    def _tail_enqueued(self, k):
        def mark():
            done = torch.cuda.Event()
            done.record(self.side_stream)
            self.tail_done[k] = done
        self._host(mark)

    def _new_logits(self, shape, dtype, pipe, numel=None):
        """Allocate the tensor the caller receives (the one per-call allocation), on the stream that writes it."""
        def alloc():
            if pipe:
                with torch.cuda.stream(self.side_stream):
                    t = torch.empty(numel if numel is not None else shape, device=self.device, dtype=dtype)
            else:
                t = torch.empty(numel if numel is not None else shape, device=self.device, dtype=dtype)
            self._tape_logits = t if numel is None else t[: shape[0] * shape[1] * shape[2]].view(shape)
            return t
        return self._host(alloc, produces=True)

    def run(self, model, x, taps=None, pipelined=False, _capturing=False, group=None):
        """``_enqueue`` + the hand-over of a one-launch recurrence's status slot to the handle a pipelined forward returns.
        ``group`` = (g, n): this pipelined forward is the g-th of a TAIL GROUP of n forwards of the same shape enqueued back to back
        through this plan -- their LSTM + head run as ONE recurrence over n x batch utterances behind the last of them."""
        self._seq_last = None
        out = self._enqueue(model, x, taps, pipelined, _capturing, group)
        if self._seq_last is not None and isinstance(out, PendingLogits):
            out._seq = (self,) + self._seq_last
        return out

    def _enqueue(self, model, x, taps=None, pipelined=False, _capturing=False, group=None):
        """Enqueue one forward of ``model`` (its parameters are read now, so a DataParallel replica runs with its own).
        ``taps`` (a dict) receives a copy of every layer's output, keyed by the layer's index in ``model.model``, in the
        oracle's layouts ((B,C,T) for encoder layers and the LSTM).  ``pipelined``: LSTM + head go to the side stream and
        a ``PendingLogits`` is returned."""
        if x.device != self.device:
            raise hip.HipError(f'input on {x.device}, plan on {self.device}')
        if not _capturing and self.seq_status.pending and not torch.cuda.is_current_stream_capturing():
            self.check_seq()                           # (an event query is not a capturable operation)
        wdtype = model.model[0].conv.weight.dtype          # (not model.parameters(): a DataParallel replica has none)
        if x.dtype != wdtype:
            raise hip.HipError(f'input is {x.dtype} but the model\'s parameters are {wdtype}: cast one of them '
                               f'(model.to(torch.bfloat16) / x.bfloat16() for the bf16 path)')
        if x.dtype not in (torch.float32, torch.bfloat16):
            raise hip.HipError(f'input must be float32 or bfloat16 (got {x.dtype})')
        x = x.detach().contiguous()
        group = self._group_or_none(model, x, taps, pipelined, _capturing, group)
        from . import walk
        key = None
        if self.tape_mode and taps is None and not _capturing and self.timer is None:
            key = tape.tape_key(self, model, x, pipelined, group)
        return self.tapes.run(self, key, model, x, pipelined, group, lambda: walk.run(self, model, x, taps, pipelined, _capturing, group))

    def _group_or_none(self, model, x, taps, pipelined, capturing, group):
        """The tail group this forward can really run in: fp32, a pipelined tail on the side stream, the fp16-pair per-frame recurrence
        and the packed input projection (the defaults), n x batch utterances within the recurrence's workspace form."""
        if group is None or group[1] <= 1 or not pipelined or taps is not None or capturing or x.dtype != torch.float32:
            return None
        from .model import LSTM_HIDDEN
        if not (model.use_rnn and self._tail_on_side_stream(x.shape[0]) and self.linear_mode == 'f16x2' and self.lstm_seq_mode in ('auto', 'frames')
                and isinstance(model.model[-1], torch.nn.Linear) and isinstance(model.model[-2], torch.nn.LSTM)
                and hip.lstm_xcd_workspace_bytes(group[1] * x.shape[0], LSTM_HIDDEN)):
            return None
        return (int(group[0]), int(group[1]))

    def _group_member(self, group, logits_all):
        """The handle of the forward just enqueued as member ``group`` = (g, n); the last member hands every handle its rows."""
        g, n = group
        if g == 0:
            self._group_handles = []
        handle = GroupLogits()
        self._group_handles.append(handle)
        if g == n - 1:
            if len(self._group_handles) != n or logits_all is None:
                raise hip.HipError(f'tail group of {n}: {len(self._group_handles)} forwards were enqueued through this plan before its last one')
            rows, done = logits_all.shape[0] // n, self.tail_done[self._turn]
            for j, h in enumerate(self._group_handles):
                h._set(logits_all[j * rows:(j + 1) * rows], done)
            self._group_handles = []
        return handle

    def _f32(self, param):
        """fp32 copy of a (bf16) parameter, rebuilt when it changes: the kernels read weights of the node ops, biases,
        gamma / beta and the LSTM / head matrices as fp32 whatever the storage type of the activations (exact: every bf16
        value is an fp32 value)."""
        if param.dtype == torch.float32:
            return param.detach()
        return self._cached(param, 'f32', lambda: param.detach().float().contiguous())


class PlanPool:
    """Idle ``ForwardPlan``s of one model, per device.  ``acquire`` hands a plan to exactly one caller at a time, so
    concurrent forwards (``torch.nn.DataParallel`` worker threads -- one per device, or several on one device) never share
    workspaces, while back-to-back calls from one thread keep re-using the same plan (LIFO).  Replicas made by
    ``nn.Module._replicate_for_data_parallel`` share this object (shallow ``__dict__`` copy); that is fine because a plan
    holds no reference to a model -- the model is an argument of every run."""

    def __init__(self):
        self._lock = threading.Lock()
        self._idle = {}              # device index -> [ForwardPlan]

    def __reduce__(self):
        return (PlanPool, ())            # copies / pickles of a model start with an empty pool

    def acquire(self, device):
        """An idle plan for a forward on ``device``'s CURRENT stream.  A plan is handed back (``release``) as soon as its forward has been
        ENQUEUED: its workspaces are still being read and written by that stream.  The same stream takes it again for free (stream
        order); another stream (two threads running forwards on two streams of one device: round 6, `bench.py --in-flight`) gets a plan
        of its own if it can -- the launch tapes of a plan are per stream as well -- and otherwise the least recently released one,
        behind the event ``release`` recorded and behind that plan's pipelined tails (round 6: before, such a plan was re-used at once
        and the two streams raced on its workspaces)."""
        device = torch.device(device)
        stream = torch.cuda.current_stream(device) if device.type == 'cuda' and torch.cuda.is_available() else None
        sid = stream.cuda_stream if stream is not None else None
        with self._lock:
            idle = self._idle.get(device.index)
            if idle:
                for i in range(len(idle) - 1, -1, -1):                  # most recently released first
                    if idle[i]._released_on == sid or idle[i]._released_on is None:
                        return idle.pop(i)
                if len(idle) >= self.MAX_IDLE_PER_DEVICE:               # bounded: a caller that makes a fresh stream per forward must not grow the pool for ever
                    plan = idle.pop(0)
                    if plan._released_event is not None:
                        stream.wait_event(plan._released_event)
                    plan.wait_tails()
                    return plan
        return ForwardPlan(device)

    MAX_IDLE_PER_DEVICE = 6

    def release(self, plan):
        if plan.device.type == 'cuda' and torch.cuda.is_available() and not torch.cuda.is_current_stream_capturing():
            stream = torch.cuda.current_stream(plan.device)
            if plan._released_event is None:
                plan._released_event = torch.cuda.Event()
            plan._released_event.record(stream)
            plan._released_on = stream.cuda_stream
        with self._lock:
            self._idle.setdefault(plan.device.index, []).append(plan)

    def poll(self, device):
        """Look (without waiting) at the status words of the one-launch recurrences enqueued through EVERY idle plan of ``device`` and
        raise for a finished one that timed out: with several plans per device (concurrent callers) the failing plan may not be the
        one the next forward is handed."""
        device = torch.device(device)
        with self._lock:
            for plan in self._idle.get(device.index, ()):
                if plan.seq_pending():
                    plan.check_seq()

    def values(self):
        """Idle plans, most recently used last (bench.py / tests read the last run's bookkeeping from them)."""
        with self._lock:
            return [p for idle in self._idle.values() for p in idle]

    def __len__(self):
        return len(self.values())

    def clear(self):
        with self._lock:
            plans = [p for idle in self._idle.values() for p in idle]
            self._idle = {}
        for p in plans:
            if torch.cuda.is_available():
                with torch.cuda.device(p.device):
                    p.close()
