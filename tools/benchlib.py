"""What the measuring tools under tools/ share: the policy of a measurement, in one place.

  window(fn, calls)            device milliseconds per call between two HIP events around ``calls`` consecutive calls of fn
  warm(fns, n)                 n calls of each function, then a device synchronisation
  alternate(fns, ...)          ``reps`` rounds, the functions taking turns, one window each per round: the raw lists of times
  summary(times, unit, digits) median, smallest and largest: as a dict under '<unit>', '<unit>_min', '<unit>_max', or as a tuple
  best_wall_ms(fn, reps)       the other measurement: host clock between two device synchronisations, best of ``reps``
  session_model(dev)           the model the session tools push through (bench.py's default architecture, keyed weights)
  bind_library / parent_rows / parent_ratio_rows
                               the same figure on another build of libnbasr_hip.so, taken by a child process of the tool
  need_device / emit / write_out
                               no device is an error, never a fall-back; a row is one JSON line as soon as it exists

A tool puts the repository on sys.path itself (stream_bench.py may point at another checkout) and imports this module by name."""
import ctypes
import json
import pathlib
import statistics
import subprocess
import sys
import time

import torch

ARCH = [[1, 0], [1, 0, 0], [1, 0, 0, 0]]        # bench.py's default architecture


def window(fn, calls=1):
    """Device milliseconds per call over ``calls`` consecutive calls of fn (HIP events on the current stream; launch gaps count)."""
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / calls


def warm(fns, n):
    """``n`` calls of each function (code objects, cached chains, allocator, clocks), then wait for the device."""
    for fn in fns:
        for _ in range(n):
            fn()
    torch.cuda.synchronize()


def alternate(fns, calls=1, reps=7, warmup=0, window=window):
    """One list of ``reps`` window times (ms per call) per function, the functions taking turns window by window so that a drift of the
    machine falls on all of them; ``warmup`` calls of each come first.  A caller that warms up with whole rounds drops them from the lists."""
    if warmup:
        warm(fns, warmup)
    times = [[] for _ in fns]
    for _ in range(reps):
        for t, fn in zip(times, fns):
            t.append(window(fn, calls))
    return times


def summary(times, unit=None, digits=2, scale=1.0):
    """Median, smallest and largest of ``times`` x ``scale``: the tuple, or with ``unit`` the rounded '<unit>', '<unit>_min', '<unit>_max'."""
    med, lo, hi = (scale * v for v in (statistics.median(times), min(times), max(times)))
    if unit is None:
        return med, lo, hi
    return {unit: round(med, digits), f'{unit}_min': round(lo, digits), f'{unit}_max': round(hi, digits)}


def best_wall_ms(fn, reps):
    """Best wall time (ms) of ``reps`` runs of fn, each bracketed by device synchronisations."""
    best = None
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        best = ms if best is None else min(best, ms)
    return best


def session_model(dev='cuda:0'):
    """The default architecture with keyed weights, on the device, in eval mode."""
    import nb_asr_amd as nb
    from nb_asr_amd.weights import keyed_fill_
    model = nb.get_model(ARCH, use_rnn=True, dropout_rate=0.0)
    keyed_fill_(model, seed=1235, mode='lively')
    return model.to(dev).eval()


def need_device(tool):
    if not torch.cuda.is_available():
        raise SystemExit(f'{tool} needs a HIP device: there is nothing to measure without one')


def emit(rows, row):
    """Print ``row`` as one JSON line, now, and keep it."""
    print(json.dumps(row), flush=True)
    rows.append(row)
    return row


def write_out(path, payload):
    """With --out: ``payload`` (the rows, or a dict around them) as a JSON file."""
    if path:
        pathlib.Path(path).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(path).write_text(json.dumps(payload, indent=1) + '\n')


def bind_library(path):
    """The child's side of --parent-library: make the package load the build at ``path`` and bind only what that build exports."""
    from nb_asr_amd import hip
    lib = ctypes.CDLL(path)
    for name in [n for n in hip.SIGNATURES if not hasattr(lib, n)]:
        del hip.SIGNATURES[name]
    hip.LIB_PATH = pathlib.Path(path)


def child_rows(stdout, when):
    """The rows a child printed (the lines that start with '{'), their library named as the parent's, ``when`` = 'before' or 'after'."""
    rows = [json.loads(line) for line in stdout.splitlines() if line.startswith('{')]
    for row in rows:
        row['library'] = f'parent ({when} this one)'
    return rows


def parent_rows(tool, library, when, argv):
    """The parent's side: run ``tool --library <library> <argv>`` as a fresh child process (a process loads one library, and one that
    has initialised the GPU never replaces its own program) and take its rows over."""
    cmd = [sys.executable, str(pathlib.Path(tool).resolve()), '--library', library, *argv]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if out.returncode != 0:
        raise SystemExit(f'the child measuring {library} failed:\n{out.stdout}\n{out.stderr}')
    rows = []
    for row in child_rows(out.stdout, when):
        emit(rows, row)
    return rows


def parent_ratio_rows(rows, batches, plain):
    """Per batch: this library's ``plain`` session (its 'session' label) over the mean of the parent's legs, and the yardstick beside
    it: the larger of the parent's own legs over the smaller."""
    mine = {r['batch']: r['us'] for r in rows if r.get('session') == plain and r['library'] == 'this'}
    out = []
    for b in batches:
        legs = [r['us'] for r in rows if r.get('session') and r['library'].startswith('parent') and r['batch'] == b]
        parent = statistics.mean(legs)
        out.append({'what': 'plain push, this library over the parent\'s', 'batch': b, 'parent_us': round(parent, 2),
                    'ratio': round(mine[b] / parent, 4), 'parent_legs_ratio': round(max(legs) / min(legs), 4)})
    return out
