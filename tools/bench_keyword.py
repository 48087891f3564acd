"""Cost of the keyword spotter (ctc.spot_keywords / KeywordStream, nbasr_ctc_keyword_step; StreamingSession(keywords=)) on one GPU:

  (a) us per StreamingSession.push of 40 feature frames (10 logit frames a push) at B in {1, 16}, with and without ``keywords=`` (8
      keywords), the two sessions alternating window by window -- and, with --parent-library, the same push without ``keywords=`` on
      another build of the library (the parent commit's), measured by a child process of this tool before and after the windows of
      this one;
  (b) us per KeywordStream.push -- the step alone -- at B in {1, 16} x {1, 8, 64} keywords x {4, 250} frames.

    python tools/bench_keyword.py [--pushes 50] [--reps 7] [--parent-library PATH] [--out profiles/streaming/keyword_bench.json]

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
SESSION_KEYWORDS = 8


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


def keyword_set(count, dev, seed=0):
    """``count`` keywords of 2 to 12 phonemes (one of them of 32), the default (untuned) thresholds."""
    gen = torch.Generator().manual_seed(seed)
    words = [torch.randint(1, 49, (int(torch.randint(2, 13, (1,), generator=gen)),), generator=gen).tolist() for _ in range(count)]
    words[-1] = torch.randint(1, 49, (32,), generator=gen).tolist()
    return ctc.KeywordSet(words, device=dev)


def session_rows(args, batches, library, with_keywords):
    """(a): the push of a session in steady state (it has emitted frames: every push commits 10 more)."""
    dev = 'cuda:0'
    model = nb.get_model(ARCH, use_rnn=True, dropout_rate=0.0)
    keyed_fill_(model, seed=1235, mode='lively')
    model = model.to(dev).eval()
    rows = []
    with torch.no_grad():
        for b in batches:
            chunk = torch.randn(b, streaming.FEATURES, CHUNK, generator=torch.Generator().manual_seed(b)).to(dev)
            kinds = [('without keywords=', {})] + ([('with keywords=', {'keywords': keyword_set(SESSION_KEYWORDS, dev)})] if with_keywords else [])
            sessions = [streaming.StreamingSession(model, b, max_chunk=CHUNK, **kw) for _, kw in kinds]
            for s in sessions:                   # past the lookahead
                for _ in range(s.lookahead_frames // CHUNK + 2):
                    s.push(chunk)
            results = alternate([lambda s=s: s.push(chunk) for s in sessions], args.pushes, args.reps)
            for (kind, _), r in zip(kinds, results):
                rows.append({'what': 'StreamingSession.push', 'session': kind, 'library': library, 'batch': b, 'frames_per_push': CHUNK, **r})
                print(json.dumps(rows[-1]), flush=True)
            if with_keywords:
                rows.append({'what': 'added by keywords=', 'library': library, 'batch': b, 'keywords': SESSION_KEYWORDS,
                             'us': round(results[1]['us'] - results[0]['us'], 2), 'ratio': round(results[1]['us'] / results[0]['us'], 4)})
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
        raise SystemExit('bench_keyword.py needs a HIP device: there is nothing to measure without one')
    batches = [int(v) for v in args.batches.split(',')]
    if args.library:                             # an older build: bind what it exports, measure what it can do
        lib = ctypes.CDLL(args.library)
        for name in [n for n in hip.SIGNATURES if not hasattr(lib, n)]:
            del hip.SIGNATURES[name]
        hip.LIB_PATH = pathlib.Path(args.library)
        session_rows(args, batches, args.library, with_keywords=False)
        return
    dev = 'cuda:0'
    rows = parent_rows(args, 'before') if args.parent_library else []
    rows += session_rows(args, batches, 'this', with_keywords=True)
    if args.parent_library:
        rows += parent_rows(args, 'after')
        plain = {r['batch']: r['us'] for r in rows if r.get('session') == 'without keywords=' and r['library'] == 'this'}
        for b in batches:
            legs = [r['us'] for r in rows if r.get('session') and r['library'].startswith('parent') and r['batch'] == b]
            parent = statistics.mean(legs)
            rows.append({'what': 'plain push, this library over the parent\'s', 'batch': b, 'parent_us': round(parent, 2),
                         'ratio': round(plain[b] / parent, 4), 'parent_legs_ratio': round(max(legs) / min(legs), 4)})
            print(json.dumps(rows[-1]), flush=True)
    # (b) the step alone
    gen = torch.Generator().manual_seed(0)
    for b in batches:
        for count in (1, 8, 64):
            keywords = keyword_set(count, dev, seed=count)
            for n in (4, 250):
                chunk = torch.randn(b, n, 49, generator=gen).to(dev)
                kw = ctc.KeywordStream(b, keywords, dev)
                (r,) = alternate([lambda: kw.push(chunk)], args.pushes, args.reps)
                rows.append({'what': 'KeywordStream.push', 'batch': b, 'keywords': count, 'frames': n, **r})
                print(json.dumps(rows[-1]), flush=True)
    if args.out:
        pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(args.out).write_text(json.dumps(rows, indent=1) + '\n')


if __name__ == '__main__':
    main()
