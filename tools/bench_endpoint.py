"""Cost of the endpointer (ctc.endpoint / EndpointStream, nbasr_ctc_endpoint_step; StreamingSession(endpoint=)) on one GPU:

  (a) ms per StreamingSession.push of 40 feature frames (10 logit frames a push) at B in {1, 16}, with and without ``endpoint=``, the
      two sessions alternating window by window -- and, with --parent-library, the same push without ``endpoint=`` on another build of
      the library (the parent commit's), measured by a child process of this tool before and after the windows of this one;
  (b) us per ctc.endpoint on (64, 250, 49) logits, with the bytes it reads over that time;
  (c) us per EndpointStream.push -- the step alone -- of 1, 10 and 40 frames at B in {1, 16}.

    python tools/bench_endpoint.py [--pushes 50] [--reps 7] [--parent-library PATH] [--out profiles/streaming/endpoint_bench.json]

Every figure is device time between two HIP events around ``--pushes`` consecutive calls (so launch gaps count, as they do for a user),
after a warm-up pass over the same shapes; the median of ``--reps`` such windows, with the smallest and largest next to it.  One JSON
line per configuration; with --out also the list as a JSON file.  There is no CPU path: without a HIP device this fails."""
import argparse
import ctypes
import json
import pathlib
import statistics
import subprocess
import sys

REPO = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

import torch                                     # noqa: E402

import nb_asr_amd as nb                          # noqa: E402
from nb_asr_amd import ctc, hip, streaming       # noqa: E402
from nb_asr_amd.weights import keyed_fill_       # noqa: E402

ARCH = [[1, 0], [1, 0, 0], [1, 0, 0, 0]]        # bench.py's default architecture
CHUNK = 40                                       # feature frames a push: 0.4 s of audio, 10 logit frames


def window_us(fn, calls):
    """Device microseconds per call over ``calls`` consecutive calls of fn (HIP events on the current stream)."""
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        fn()
    stop.record()
    stop.synchronize()
    return 1e3 * start.elapsed_time(stop) / calls


def summary(times, digits=2):
    return {'us': round(statistics.median(times), digits), 'us_min': round(min(times), digits), 'us_max': round(max(times), digits)}


def alternate(fns, calls, reps):
    """One summary per function over ``reps`` windows each, the functions taking turns."""
    for fn in fns:
        fn()
        fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            times[i].append(window_us(fn, calls))
    return [summary(t) for t in times]


def session_rows(args, batches, library, with_endpoint):
    """(a): the push of a session in steady state (it has emitted frames: every push commits 10 more)."""
    dev = 'cuda:0'
    model = nb.get_model(ARCH, use_rnn=True, dropout_rate=0.0)
    keyed_fill_(model, seed=1235, mode='lively')
    model = model.to(dev).eval()
    rows = []
    with torch.no_grad():
        for b in batches:
            chunk = torch.randn(b, streaming.FEATURES, CHUNK, generator=torch.Generator().manual_seed(b)).to(dev)
            kinds = [('without endpoint=', {})] + ([('with endpoint=', {'endpoint': ctc.EndpointRules(device=dev)})] if with_endpoint else [])
            sessions = [streaming.StreamingSession(model, b, max_chunk=CHUNK, **kw) for _, kw in kinds]
            for s in sessions:                   # past the lookahead
                for _ in range(s.lookahead_frames // CHUNK + 2):
                    s.push(chunk)
            results = alternate([lambda s=s: s.push(chunk) for s in sessions], args.pushes, args.reps)
            for (kind, _), r in zip(kinds, results):
                rows.append({'what': 'StreamingSession.push', 'session': kind, 'library': library, 'batch': b, 'frames_per_push': CHUNK, **r})
                print(json.dumps(rows[-1]), flush=True)
            if with_endpoint:
                rows.append({'what': 'added by endpoint=', 'library': library, 'batch': b, 'us': round(results[1]['us'] - results[0]['us'], 2),
                             'ratio': round(results[1]['us'] / results[0]['us'], 4)})
                print(json.dumps(rows[-1]), flush=True)
    return rows


def parent_rows(args, when):
    """(a) on another build of the library, in a child process of this tool (a process loads one library)."""
    cmd = [sys.executable, str(pathlib.Path(__file__).resolve()), '--library', args.parent_library, '--pushes', str(args.pushes), '--reps',
           str(args.reps), '--batches', args.batches]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if out.returncode != 0:
        raise SystemExit(f'the child measuring {args.parent_library} failed:\n{out.stdout}\n{out.stderr}')
    rows = [json.loads(line) for line in out.stdout.splitlines() if line.startswith('{')]
    for row in rows:
        row['library'] = f'parent ({when} this one)'
        print(json.dumps(row), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pushes', type=int, default=50)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--batches', default='1,16')
    ap.add_argument('--parent-library', default=None, help='another libnbasr_hip.so to measure the plain push on (the parent commit\'s)')
    ap.add_argument('--library', default=None, help='measure ONLY the plain push, on this library (what --parent-library starts)')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_endpoint.py needs a HIP device: there is nothing to measure without one')
    batches = [int(v) for v in args.batches.split(',')]
    if args.library:                             # an older build: bind what it exports, measure what it can do
        lib = ctypes.CDLL(args.library)
        for name in [n for n in hip.SIGNATURES if not hasattr(lib, n)]:
            del hip.SIGNATURES[name]
        hip.LIB_PATH = pathlib.Path(args.library)
        session_rows(args, batches, args.library, with_endpoint=False)
        return
    dev = 'cuda:0'
    rows = parent_rows(args, 'before') if args.parent_library else []
    rows += session_rows(args, batches, 'this', with_endpoint=True)
    if args.parent_library:
        rows += parent_rows(args, 'after')
        plain = {r['batch']: r['us'] for r in rows if r.get('session') == 'without endpoint=' and r['library'] == 'this'}
        for b in batches:
            parent = statistics.mean(r['us'] for r in rows if r.get('session') and r['library'].startswith('parent') and r['batch'] == b)
            rows.append({'what': 'plain push, this library over the parent\'s', 'batch': b, 'parent_us': round(parent, 2), 'ratio': round(plain[b] / parent, 4)})
            print(json.dumps(rows[-1]), flush=True)
    gen = torch.Generator().manual_seed(0)
    rules = ctc.EndpointRules(device=dev)
    # (b) whole utterances
    x = torch.randn(64, 250, 49, generator=gen).to(dev)
    (r,) = alternate([lambda: ctc.endpoint(x, None, rules)], args.pushes, args.reps)
    row = {'what': 'ctc.endpoint', 'shape': list(x.shape), **r, 'bytes': x.numel() * 4}
    row['gb_per_s'] = round(row['bytes'] / row['us'] / 1e3, 1)
    rows.append(row)
    print(json.dumps(row), flush=True)
    # (c) the step alone
    for b in batches:
        for n in (1, 10, 40):
            chunk = torch.randn(b, n, 49, generator=gen).to(dev)
            ep = ctc.EndpointStream(b, rules, dev)
            (r,) = alternate([lambda: ep.push(chunk)], args.pushes, args.reps)
            rows.append({'what': 'EndpointStream.push', 'batch': b, 'frames': n, **r})
            print(json.dumps(rows[-1]), flush=True)
    if args.out:
        pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(args.out).write_text(json.dumps(rows, indent=1) + '\n')


if __name__ == '__main__':
    main()
