"""The status words of the one-launch LSTM recurrences enqueued through a plan: who reads them, when, and who reports a failure.

A resident recurrence can time out when another process takes its compute units; its logits then hold NaN rows.  Behind every such launch
its status word travels to pinned host memory, stream-ordered and without a host synchronisation (ADVICE r3 / VERDICT r3 next 6: the word
used to be read by nobody).  The rules, all kept by ``SeqStatusRing``:

* one pinned word PER LAUNCH (a ring): a caller may enqueue many forwards before anything is looked at, and the next launch clears the
  device-side word -- a single host word would let a later, healthy forward overwrite an earlier one's timeout;
* a slot about to be re-used still holds an unread word: it is read first;
* a verdict consumed by the poll (the next forward's look, or the ring wrap) is remembered per slot, so the handle of exactly that forward
  still reports it from its ``result()``, once (it used to return NaN logits silently then);
* ``PendingLogits.result()`` may run on another thread than the one enqueueing through the plan: every operation takes the lock.
"""
import collections
import threading

import torch


class SeqStatusRing:
    SIZE = 256

    def __init__(self):
        self.host = None                     # the pinned ring of status words (allocated with the first launch)
        self.pending = collections.deque()   # (event behind the status copy, slot) of the launches nobody has looked at yet
        self.slot, self.failed = 0, False    # the next launch's slot / a failure the poll has seen and not yet reported
        self.outcome = {}                    # slot -> whether that launch failed, once the poll has read its word
        self.lock = threading.Lock()

    def launched(self, ws, device):
        """A one-launch recurrence was enqueued on ``device``'s current stream with its status word at the start of ``ws``:
        (event behind the copy of that word, ring slot)."""
        if self.host is None:
            self.host = torch.zeros(self.SIZE, dtype=torch.int32).pin_memory()
        with self.lock:
            if len(self.pending) >= self.SIZE:                # the slot about to be re-used still holds an unread word: read it first
                ev, slot = self.pending.popleft()
                ev.synchronize()
                self._note(slot)
            slot = self.slot
            self.outcome.pop(slot, None)                      # (a new launch takes the slot: its old verdict is history)
            self.slot = (slot + 1) % self.SIZE
            ev = self._copy(ws, slot, device)
            self.pending.append((ev, slot))
        return ev, slot

    def _copy(self, ws, slot, device):
        self.host[slot: slot + 1].copy_(ws.view(torch.int32)[:1], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(device))
        return ev

    def _note(self, slot):
        """The verdict of the launch behind ring slot ``slot`` (its status copy has landed): latched for the next poll's caller
        (``failed``) AND remembered per slot for ``verdict``."""
        failed = int(self.host[slot]) != 0
        self.outcome[slot] = failed
        self.failed |= failed

    def poll(self, wait=False):
        """Read the words of the finished launches (``wait``: of every launch, blocking until it has finished) and say, once, whether
        one of the launches read so far failed."""
        pending = self.pending
        with self.lock:
            while pending:
                ev, slot = pending[0]
                if wait:
                    ev.synchronize()
                elif not ev.query():
                    break
                pending.popleft()
                self._note(slot)
            failed, self.failed = self.failed, False
        return failed

    def verdict(self, ev, slot):
        """Wait for ONE launch (the status copy behind it) and say whether it failed."""
        ev.synchronize()
        with self.lock:
            try:
                self.pending.remove((ev, slot))               # reported by its own forward, not again by the next poll
                failed = int(self.host[slot]) != 0
            except ValueError:
                # the poll or the ring wrap has consumed the word already: its verdict was recorded per slot
                failed = bool(self.outcome.pop(slot, False))
                if failed:
                    self.failed = False                       # reported by the forward it belongs to
        return failed
