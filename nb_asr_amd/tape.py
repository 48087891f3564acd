"""Launch tapes: the enqueueing C-ABI calls of one forward, recorded once and replayed for every later call with the same key.

``LaunchTape`` is one recorded sequence; ``Tapes`` is what a ``ForwardPlan`` owns -- the tapes by key, the seen-twice counter, the
mutation count that decides whether a recording may be kept, and the ONE ``invalidate()`` everything that moves a workspace, rebuilds a
derived weight or changes the plan's route goes through.  ``tape_key`` is everything a recorded sequence depends on.
"""
import os
import weakref

import torch

from . import hip


# Any submodule or parameter (re-)registered on any module bumps this counter: a launch tape recorded before is not replayed
# afterwards (a layer swapped inside a model that has already run must be seen by the next forward).
_structure_epoch = [0]


def _bump_structure_epoch(*_args):
    _structure_epoch[0] += 1


torch.nn.modules.module.register_module_module_registration_hook(_bump_structure_epoch)
torch.nn.modules.module.register_module_parameter_registration_hook(_bump_structure_epoch)


class LaunchTape:
    """The enqueueing C-ABI calls of ONE forward, recorded once and replayed for every later batch with the same key
    (shape, dtype, streams, parameter addresses and versions): the plan's workspaces and the derived weight copies sit
    at fixed addresses, so the only arguments that change are the caller's input pointer and the freshly allocated
    logits, which are patched into the recorded argument lists.  Host-side steps that belong to the sequence (event
    record / wait between the main and the side stream, the logits allocation) are recorded as callables.

    Why: a forward is ~380 launches, ~130 of them issued from python at ~12 us each; at 8 utterances per GPU (the
    strong-scaling split of the benchmark batch) that host time, 2.4 ms, exceeds the device time.  A replay issues the same
    calls in ~0.4 ms (tools/ubench/host_issue.py)."""

    def __init__(self, entries, x_ptr, pipelined, pipe, group=None):
        self.entries, self.pipelined, self.pipe, self.group = entries, pipelined, pipe, group
        self.x_slots = []
        producers = [(i, e) for i, e in enumerate(entries) if e[0] is None and e[2] is not None]
        for i, e in enumerate(entries):
            if e[0] is None:
                continue
            for j, a in enumerate(e[1]):
                if type(a) is not int:
                    continue
                if a == x_ptr:
                    self.x_slots.append((i, j))
                for pi, pe in producers:
                    if pi < i and a == pe[2]:
                        pe[3].append((i, j))
        self.launches = sum(1 for e in entries if e[0] is not None)

    def replay(self, plan, x):
        entries = self.entries
        if not self.pipe:
            plan.wait_tails()
        px = x.data_ptr()
        for i, j in self.x_slots:
            entries[i][1][j] = px
        for e in entries:
            fn = e[0]
            if fn is None:
                t = e[1]()
                if e[3]:
                    p = t.data_ptr()
                    for i, j in e[3]:
                        entries[i][1][j] = p
            else:
                rc = fn(*e[1])
                if rc:
                    hip._check(rc, fn.__name__)
        logits, plan._tape_logits = plan._tape_logits, None
        if self.group is not None:
            return plan._group_member(self.group, logits)
        if self.pipelined:
            from .executor import PendingLogits          # (executor imports this module)
            return PendingLogits(logits, plan.tail_done[plan._turn] if self.pipe else None)
        return logits


_TAPE_ENV = ('NBASR_GC_F32_VARIANT',)       # (NBASR_LSTM_SEQ and the other plan switches are read once, when the plan is built)


def tape_key(plan, model, x, pipelined, group=None):
    """Everything the recorded launch sequence depends on; None: this call cannot use a tape."""
    if getattr(model, '_is_replica', False) or x.numel() == 0:    # DataParallel replica: its weights are fresh tensors every step
        return None
    tapes = plan.tapes
    slots, epoch = tapes.param_slots, _structure_epoch[0]
    if slots is None or slots[0]() is not model or slots[2] != epoch:
        found = [(m._parameters, n) for m in model.modules() for n, p in m._parameters.items() if p is not None]
        slots = tapes.param_slots = (weakref.ref(model), found, epoch)
    params = tuple([(d[n].data_ptr(), d[n]._version) for d, n in slots[1]])
    pipe = bool(pipelined) and model.use_rnn and plan._tail_on_side_stream(x.shape[0])
    slot = -1 if not pipe else (plan._turn ^ 1) if (group is None or group[0] == 0) else plan._turn      # (a group's first forward rotates the slot)
    return (x.dtype, tuple(x.shape), x.data_ptr() % 16 == 0, bool(pipelined), slot, group,
            torch.cuda.current_stream(plan.device).cuda_stream, tuple(os.environ.get(k) for k in _TAPE_ENV),
            epoch, tuple(map(id, model.model)), params, structure_fingerprint(model))


def structure_fingerprint(model):
    """The PLAIN attributes the launch sequence reads on every call and that no registration hook sees:
    ``node.branch_ops`` is a python list, ``cell.use_norm`` / ``op.dilation`` / ``norm.eps`` / ``model.use_rnn`` are plain
    attributes -- mutating one after a tape exists must not replay the old sequence."""
    fp = [model.use_rnn, model.training, getattr(model, 'dropout_rate', 0.0)]
    for layer in model.model:
        nodes = getattr(layer, 'nodes', None)
        if nodes is not None:
            fp.append(layer.use_norm)
            fp.append(layer.norm_layer.eps if layer.use_norm else None)
            for node in nodes:
                op = node.op
                fp.append((type(op), getattr(op, 'kernel_size', 0), getattr(op, 'dilation', 0), getattr(op, 'groups', 0),
                           tuple(map(type, node.branch_ops))))
        else:
            fp.append((type(layer), getattr(layer, 'eps', None), getattr(layer, 'kernel_size', 0), getattr(layer, 'strides', 0),
                       getattr(layer, 'groups', 0), getattr(layer, 'p', None)))
    return tuple(fp)


class Tapes:
    """The launch tapes of one plan and the decision between issuing a forward from python, recording it and replaying it."""

    def __init__(self):
        self.tapes, self.seen = {}, {}       # key -> LaunchTape / how often the key has come by
        self.recording = None                # the entries list while a tape is being recorded (ForwardPlan._host appends host steps)
        self.mutations = 0                   # workspace growths, derived-weight rebuilds, demotions: any of them while recording, and the tape is not kept
        self.replays = 0
        self.param_slots = None              # tape_key: (weakref(model), [(module._parameters, name), ...], structure epoch)

    def invalidate(self):
        """No recorded sequence is valid any more -- neither the stored ones nor one that is being recorded right now (possibly by
        another thread: ``PendingLogits.result()`` demotes the plan from whichever thread reads the result)."""
        self.tapes.clear()
        self.mutations += 1

    def run(self, plan, key, model, x, pipelined, group, body):
        """The result of ``body()`` -- or of the replay of the tape recorded for ``key`` (None: this call cannot use one)."""
        if key is None:
            return body()
        tape = self.tapes.get(key)
        if tape is not None:
            self.replays += 1
            return tape.replay(plan, x)
        if len(self.seen) > 256:
            self.seen.clear()
        seen = self.seen[key] = self.seen.get(key, 0) + 1
        if seen < 2:
            # first sight of this key: workspaces may grow and derived weights may be built -- not a sequence worth keeping
            return body()
        entries, before = [], self.mutations
        self.recording = entries
        hip.start_tape(entries)
        try:
            out = body()
        finally:
            hip.stop_tape()
            self.recording = None
        if self.mutations == before:
            if len(self.tapes) >= 48:               # (a tail group of 8 on two slots: 16 tapes of one shape)
                self.tapes.clear()
            self.tapes[key] = LaunchTape(entries, x.data_ptr(), bool(pipelined),
                                         bool(pipelined) and model.use_rnn and plan._tail_on_side_stream(x.shape[0]), group)
        plan._tape_logits = None
        return out
