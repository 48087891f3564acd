"""Cost of the confidence step on one GPU (ctc.confidence / ConfidenceStream, nbasr_ctc_confidence_step; StreamingSession(confidence=)):
us per ConfidenceStream.push -- the step alone -- on (64, n, 49) logits at n in {1, 10, 40, 250}, for each measure, beside
hip.ctc_greedy_stream on the same logits: nbasr_ctc_greedy_stream is the existing kernel that reads the same logits once, the yardstick
(no target is set).  The calls take turns window by window, in one process on one library.

    python tools/bench_confidence.py [--pushes 50] [--reps 7] [--batch 64] [--frames 1,10,40,250] [--out profiles/streaming/confidence_bench.json]

Every figure is device time between two HIP events around ``--pushes`` consecutive calls (so launch gaps count, as they do for a user),
after a warm-up pass over the same shapes; the median of ``--reps`` such windows, with the smallest and largest next to it.  One JSON
line per configuration; with --out also the list as a JSON file.  There is no CPU path: without a HIP device this fails."""
import argparse
import pathlib
import sys

REPO = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

import torch                                     # noqa: E402

import benchlib                                  # noqa: E402
from nb_asr_amd import ctc, hip                  # noqa: E402

WARMUP = 2                                       # calls of each function before its windows
CLASSES = 49


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--pushes', type=int, default=50)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--frames', default='1,10,40,250')
    ap.add_argument('--out', default=None)
    args = ap.parse_args(argv)
    benchlib.need_device('bench_confidence.py')
    dev, b, rows = 'cuda:0', args.batch, []
    gen = torch.Generator().manual_seed(0)
    for n in (int(v) for v in args.frames.split(',')):
        chunk = (torch.randn(b, n, CLASSES, generator=gen) * 3).to(dev)
        prev = torch.full((b,), -1, dtype=torch.int32, device=dev)
        streams = [ctc.ConfidenceStream(b, ctc.ConfidenceRules(measure, device=dev), dev) for measure in ctc.CONFIDENCE_MEASURES]
        fns = [lambda: hip.ctc_greedy_stream(chunk, prev)] + [lambda s=s: s.push(chunk) for s in streams]
        results = [benchlib.summary(t, 'us', scale=1e3) for t in benchlib.alternate(fns, args.pushes, args.reps, warmup=WARMUP)]
        benchlib.emit(rows, {'what': 'hip.ctc_greedy_stream', 'batch': b, 'frames': n, 'classes': CLASSES, **results[0]})
        for s, r in zip(streams, results[1:]):
            benchlib.emit(rows, {'what': 'ConfidenceStream.push', 'measure': s.rules.measure, 'batch': b, 'frames': n, 'classes': CLASSES, **r,
                                 'over_greedy': round(r['us'] / results[0]['us'], 3)})
    benchlib.write_out(args.out, rows)
    return rows


if __name__ == '__main__':
    main()
