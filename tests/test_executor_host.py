"""Host logic of the executor that needs no GPU: launch-tape argument patching, the node-kernel variant table, tape keys."""
import json
import pathlib

import pytest
import torch
import torch.nn as nn

import cases
import nb_asr_amd as nb
from nb_asr_amd import executor, hip, tiles


class _Ptr:
    """Stands in for a tensor whose address a tape patches."""

    def __init__(self, p):
        self.p = p

    def data_ptr(self):
        return self.p


def test_launch_tape_patches_the_input_and_produced_tensors():
    calls = []

    def fn_a(*args):
        calls.append(('a', args))
        return 0

    def fn_b(*args):
        calls.append(('b', args))
        return 0
    fn_a.__name__, fn_b.__name__ = 'fn_a', 'fn_b'
    produced = iter([_Ptr(0x9000), _Ptr(0xA000)])
    x0, logits0 = 0x1000, 0x7000
    entries = [
        [fn_a, [x0, 0x2000, 64, 3, None, 0.5]],                      # reads the input
        [None, lambda: next(produced), logits0, []],                 # host step that allocates the logits
        [fn_b, [0x2000, logits0, 49, x0]],                           # writes them (and reads x again)
        [fn_a, [0x3000, logits0, 7, 1, None, 1.0]],
    ]
    tape = executor.LaunchTape(entries, x0, pipelined=False, pipe=False)
    assert tape.x_slots == [(0, 0), (2, 3)] and entries[1][3] == [(2, 1), (3, 1)] and tape.launches == 3

    class Plan:
        _tape_logits = 'logits'
        tail_done = [None, None]
        _turn = 0

        def wait_tails(self):
            calls.append(('wait', ()))
    plan = Plan()
    assert tape.replay(plan, _Ptr(0x5000)) == 'logits' and plan._tape_logits is None
    assert calls == [('wait', ()), ('a', (0x5000, 0x2000, 64, 3, None, 0.5)), ('b', (0x2000, 0x9000, 49, 0x5000)),
                     ('a', (0x3000, 0x9000, 7, 1, None, 1.0))]
    calls.clear()
    plan._tape_logits = 'again'
    tape.replay(plan, _Ptr(0x6000))
    assert calls[1] == ('a', (0x6000, 0x2000, 64, 3, None, 0.5)) and calls[2] == ('b', (0x2000, 0xA000, 49, 0x6000))
    # small integers that happen to equal nothing are never patched: 64, 3, 49, 7 above stayed what they were


def test_launch_tape_reports_a_failing_call(monkeypatch):
    def bad(*args):
        return -1
    bad.__name__ = 'nbasr_something'
    monkeypatch.setattr(hip, '_check', lambda rc, what: (_ for _ in ()).throw(hip.HipError(f'{what} failed with code {rc}')))
    tape = executor.LaunchTape([[bad, [1, 2]]], 0x1000, False, False)

    class Plan:
        _tape_logits = None
        tail_done = [None, None]
        _turn = 0

        def wait_tails(self):
            pass
    with pytest.raises(hip.HipError, match='nbasr_something failed with code -1'):
        tape.replay(Plan(), _Ptr(0x1000))


def test_variant_table_is_complete_and_well_formed():
    table = json.loads(pathlib.Path(tiles.__file__).with_name('gc_variant_table.json').read_text())
    # (taps, dilation) x channels per group x {4 flavours + 2 statistics flavours} x {small, large}
    assert table == tiles._GC_TABLE and len(table) == 4 * 4 * (4 + 2) * 2
    no_split = (0, hip.GC_PIPE, hip.GC_RING)
    for key, v in table.items():
        parts = key.split(',')
        k, d, cg = map(int, parts[:3])
        assert (k, d) in ((5, 1), (5, 2), (7, 1), (7, 2)) and cg in (6, 8, 10, 12)
        assert parts[3] in ('lnx', 'lnx+skip', 'skip', 'plain') and parts[4] in ('small', 'large')
        if len(parts) == 6:
            assert parts[5] == 'stats' and parts[3] in ('plain', 'skip') and v in no_split      # statistics launches: no output split
        else:
            assert v in no_split + (hip.GC_OSPLIT, hip.GC_PIPE | hip.GC_OSPLIT)
    # every key has been measured in profiles/: the table is a function of the committed logs
    logs = list((pathlib.Path(__file__).resolve().parent.parent / 'profiles' / 'r03_gc_variants').glob('*.jsonl'))
    rows = [json.loads(line) for f in logs for line in f.read_text().splitlines() if line.startswith('{')]
    assert len([r for r in rows if r['batch'] in (8, 64)]) == len(table)


def test_variant_choice_per_launch(monkeypatch):
    pick = lambda view, *a: tiles.gc_variant(tiles._GC_TABLE, view.shape, *a)          # noqa: E731
    model = nb.get_model(cases.ARCH_D, use_rnn=True, dropout_rate=0.0)
    cell = next(m for m in model.model if type(m).__name__ == 'SearchCell' and m.filters == 1200)
    node = cell.nodes[0]                                           # conv7d2 or similar with 12 channels per group
    op = node.op
    cg = 1200 // op.groups

    def view(b, frames):
        return torch.empty(1).as_strided((b, 1200, hip.round_up4(frames)), (0, 0, 0))        # only its shape is looked at
    has_skip = any(type(br).__name__ == 'Identity' for br in node.branch_ops)
    flavour = 'skip' if has_skip else 'plain'
    for b, frames, size in ((64, 250, 'large'), (8, 250, 'small'), (2, 40, 'small')):
        want = tiles._GC_TABLE[f'{op.kernel_size},{op.dilation},{cg},{flavour},{size}']
        assert pick(view(b, frames), node, None, None, 2) == want
        assert pick(view(b, frames), node, None, ('stats',), 2) == tiles._GC_TABLE[f'{op.kernel_size},{op.dilation},{cg},{flavour},{size},stats']
    ln0 = ('stats', 'gamma', 'beta')
    assert pick(view(64, 250), node, ln0, None, 1) == tiles._GC_TABLE[f'{op.kernel_size},{op.dilation},{cg},{"lnx+skip" if has_skip else "lnx"},large']
    assert pick(view(64, 250), None) == 0                                   # no node: the default kernel
    monkeypatch.setenv('NBASR_GC_F32_VARIANT', str(hip.GC_PIPE | hip.GC_OSPLIT))
    assert pick(view(64, 250), node, None, None, 2) == hip.GC_PIPE | hip.GC_OSPLIT
    assert pick(view(64, 250), node, None, ('stats',), 2) == hip.GC_PIPE       # the split is never forced onto a statistics launch
    monkeypatch.delenv('NBASR_GC_F32_VARIANT')
    monkeypatch.setenv('NBASR_GC_F32_VARIANT', '0')                                     # the default kernel everywhere
    assert pick(view(64, 250), node, None, None, 2) == 0


def test_structure_epoch_counts_registrations():
    before = executor._structure_epoch[0]
    m = nn.Linear(3, 3)
    assert executor._structure_epoch[0] > before                    # weight and bias were registered
    mid = executor._structure_epoch[0]
    seq = nn.Sequential(m)
    seq[0] = nn.Linear(3, 3)
    assert executor._structure_epoch[0] > mid


def test_bench_reads_only_attributes_a_plan_has():
    """bench.py reports bookkeeping of the last plan in its JSON line; a removed plan attribute must not survive there (round 3 pruned
    several switches -- the bench line is produced on the GPU box only, so this is checked here, without a GPU)."""
    import re
    root = pathlib.Path(__file__).resolve().parent.parent
    plan = executor.ForwardPlan('cpu')
    for name in sorted(set(re.findall(r'\bplan\.([A-Za-z_]+)', (root / 'bench.py').read_text()))):
        assert hasattr(plan, name), f'bench.py reads plan.{name}, which ForwardPlan does not have'


def test_removed_environment_switches_are_announced_once(monkeypatch):
    """a script that still sets a switch of rounds 1-3 (NBASR_TRAIN_GEMM became NBASR_DENSE_MODE, ...) is told so, once."""
    import warnings
    from nb_asr_amd import executor
    monkeypatch.setenv('NBASR_TRAIN_GEMM', 'f32')
    monkeypatch.setattr(executor, '_warned_removed', [False])
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter('always')
        executor._warn_removed_switches()
        executor._warn_removed_switches()
    assert len(seen) == 1 and 'NBASR_TRAIN_GEMM' in str(seen[0].message) and 'NBASR_DENSE_MODE' in str(seen[0].message)


def test_dense_mode_is_read_and_validated_at_call_time(monkeypatch):
    """hip.dense_mode() is the one reader of NBASR_DENSE_MODE (inference plan, autograd, backward): nothing cached at import, and a
    misspelt value raises in training as it does when a plan is built."""
    monkeypatch.delenv('NBASR_DENSE_MODE', raising=False)
    assert hip.dense_mode() == 'auto' and executor.ForwardPlan('cpu').dense_mode == 'auto'
    for value in ('auto', 'bf16x3', 'f32'):
        monkeypatch.setenv('NBASR_DENSE_MODE', value)
        assert hip.dense_mode() == value and executor.ForwardPlan('cpu').dense_mode == value
    for value in ('F32', 'fp32'):
        monkeypatch.setenv('NBASR_DENSE_MODE', value)
        with pytest.raises(ValueError, match=f'NBASR_DENSE_MODE must be auto, bf16x3 or f32, got {value!r}'):
            hip.dense_mode()
        with pytest.raises(ValueError, match='NBASR_DENSE_MODE must be auto, bf16x3 or f32'):
            executor.ForwardPlan('cpu')


class _Model:
    use_rnn = False


@pytest.mark.parametrize('mutation', ['demote', 'buf', 'cached', None])
def test_a_mutation_while_recording_drops_the_tape(mutation):
    """One ``invalidate()`` for everything that makes a recorded sequence stale.  A plan demoted halfway through a recording -- by
    ``PendingLogits.result()`` on another thread, say -- used to clear the stored tapes only: the tape being recorded was stored after the
    clear and replayed the resident launch the plan had just been demoted from (the tape key does not hold ``lstm_seq_mode``)."""
    plan = executor.ForwardPlan('cpu')
    tapes, param = plan.tapes, torch.zeros(3)
    plan._cached(param, 'copy', param.clone)
    calls = []

    def body():
        calls.append(tapes.recording is not None)
        if len(calls) == 2:                               # second sight of the key: this call is being recorded
            if mutation == 'demote':
                plan._demote()
            elif mutation == 'buf':
                plan._buf('grown', 1000)
            elif mutation == 'cached':
                param.add_(1.0)                           # (version counter: the derived copy is rebuilt)
                plan._cached(param, 'copy', param.clone)
        return 'out'
    run = lambda: tapes.run(plan, 'key', _Model(), _Ptr(0x1000), False, None, body)      # noqa: E731
    assert run() == 'out' and calls == [False] and not tapes.tapes                      # first sight: python, nothing kept
    assert run() == 'out' and calls == [False, True] and tapes.recording is None
    if mutation is None:                                  # the control: an undisturbed recording is kept and replayed
        assert list(tapes.tapes) == ['key'] and tapes.replays == 0
        plan._tape_logits = 'replayed'
        assert run() == 'replayed' and len(calls) == 2 and tapes.replays == 1
        return
    assert not tapes.tapes                                # no tape is stored for that key
    assert run() == 'out' and calls == [False, True, True] and tapes.replays == 0       # the next call records again, not replays
    assert list(tapes.tapes) == ['key']
    if mutation == 'demote':
        assert plan.lstm_seq_mode == 'frames'


class _Event:
    def __init__(self, done=True):
        self.done, self.waited = done, 0

    def query(self):
        return self.done

    def synchronize(self):
        self.waited += 1
        self.done = True


class _StandInRing(executor.seq_status.SeqStatusRing):
    """The ring with a list for the pinned tensor and ``_Event`` for the events: ``launched(word)`` lands ``word`` in its slot at once."""

    def __init__(self):
        super().__init__()
        self.host = [0] * self.SIZE

    def _copy(self, word, slot, device):
        self.host[slot] = word
        return _Event(done=word != 'in flight')


def _plan_with_stand_in_ring():
    plan = executor.ForwardPlan('cpu')
    plan.seq_status = _StandInRing()
    return plan, plan.seq_status


def test_status_ring_wraps_and_reads_the_evicted_slot_first():
    plan, ring = _plan_with_stand_in_ring()
    first_ev, first_slot = ring.launched(1, None)         # a failed launch nobody looks at ...
    first_ev.done = False
    handles = [ring.launched(0, None) for _ in range(ring.SIZE - 1)]
    assert [slot for _, slot in handles] == list(range(1, ring.SIZE)) and len(ring.pending) == ring.SIZE and first_ev.waited == 0
    ev, slot = ring.launched(0, None)                     # ... until the ring wraps: its word is read before the slot is taken again
    assert slot == first_slot == 0 and first_ev.waited == 1 and len(ring.pending) == ring.SIZE and ring.host[0] == 0
    assert plan.seq_pending()
    with pytest.raises(hip.HipError, match='EARLIER forward'):
        plan.check_seq()
    assert plan.lstm_seq_mode == 'frames' and not plan.seq_pending()
    plan.check_seq(wait=True)                             # reported once
    plan.check_seq_slot(ev, slot)                         # the slot's new launch is healthy: the evicted verdict is history


def test_a_failure_the_poll_consumed_is_still_raised_by_its_own_handle_once():
    plan, ring = _plan_with_stand_in_ring()
    ok = ring.launched(0, None)
    bad = ring.launched(7, None)
    late = ring.launched('in flight', None)
    with pytest.raises(hip.HipError, match='EARLIER forward'):
        plan.check_seq()                                  # the non-waiting poll reads the two finished launches
    assert list(ring.pending) == [late] and late[0].waited == 0 and plan.lstm_seq_mode == 'frames'
    with pytest.raises(hip.HipError, match='THIS forward'):
        plan.check_seq_slot(*bad)
    plan.check_seq_slot(*ok)
    plan.check_seq()                                      # not again
    plan.check_seq_slot(*bad)                             # nor by the handle
    ring.host[late[1]] = 0
    plan.check_seq(wait=True)
    assert late[0].waited == 1 and not plan.seq_pending()


def test_a_failure_first_seen_by_its_handle_is_not_reported_again():
    plan, ring = _plan_with_stand_in_ring()
    bad = ring.launched(1, None)
    ok = ring.launched(0, None)
    with pytest.raises(hip.HipError, match='THIS forward'):
        plan.check_seq_slot(*bad)
    assert list(ring.pending) == [ok] and plan.lstm_seq_mode == 'frames'
    plan.check_seq()
    plan.check_seq(wait=True)
    assert not plan.seq_pending()
