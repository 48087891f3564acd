"""Cost of training-mode dropout at p = 0.2 on one GPU, ATen's against the counter-based HIP kernel (nbasr_dropout), on op-sized tensors:
the cell widths of model.FILTERS at their frame counts for B = 64 utterances of T = 1000 frames.

  (a) torch.nn.functional.dropout(x, 0.2, True)  |  hip.dropout out of place (its output allocated per call, as ATen's is)  |  in place;
  (b) the node's sum over one and three skips: ATen's dropout then skip_sum  |  hip.dropout then skip_sum  |  the fused launch.

    python tools/bench_dropout.py [--window-ms 400] [--reps 5] [--out profiles/dropout/dropout_bench.json]

The forms of a group take turns, window by window, in one process.  Every figure is device time between two HIP events around
consecutive calls (launch gaps count, as they do for a user) after a warm-up of the same shapes; the number of calls per window is
chosen per shape so that a window lasts about --window-ms.  Reported: the median of --reps windows with the smallest and largest, and the
bytes the form must move (from the shapes: 4 per element read or written, 1 per element for ATen's saved mask) over the median.
One JSON line per form and shape; with --out also the list as a JSON file.  There is no CPU path: without a HIP device this fails."""
import argparse
import math
import pathlib
import sys

REPO = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

import torch                                     # noqa: E402

import benchlib                                  # noqa: E402
from nb_asr_amd import hip, model                # noqa: E402

P = 0.2
BATCH, FRAMES = 64, 1000


def op_shapes(batch=BATCH, frames=FRAMES):
    """(batch, width, frames at that block) for the four blocks: the downsample strides halve the frames in front of blocks 2 and 3."""
    shapes, t = [], frames
    for width, stride in zip(model.FILTERS, model.DOWN_STRIDES):
        t = (t + stride - 1) // stride
        shapes.append((batch, width, t))
    return shapes


def forms(x, skips):
    """{name: (callable, bytes per element)} of one group; ``skips`` empty: the dropout alone."""
    frames, n = x.shape[2], len(skips)
    calls = iter(range(1 << 62))

    def hip_drop(out=None, sk=()):
        return hip.dropout(x, torch.empty_like(x) if out is None else out, frames, P, 1234, next(calls), sk)

    def summed(first):
        acc = hip.skip_sum([first, *skips[:2]], torch.empty_like(x), frames)          # as autograd._SkipSum: three terms per launch
        return acc if n < 3 else hip.skip_sum([acc, skips[2]], torch.empty_like(x), frames)
    sum_bytes = 4 * (n + 2) if n < 3 else 4 * (4 + 3)          # a skip_sum launch reads its terms and writes one tensor
    if not skips:
        scratch = x.clone()
        return {'aten': (lambda: torch.nn.functional.dropout(x, P, True), 9),
                'hip': (hip_drop, 8),
                'hip_in_place': (lambda: hip.dropout(scratch, scratch, frames, P, 1234, next(calls)), 8)}
    return {f'aten_then_skip_sum_{n}': (lambda: summed(torch.nn.functional.dropout(x, P, True)), 9 + sum_bytes),
            f'hip_then_skip_sum_{n}': (lambda: summed(hip_drop()), 8 + sum_bytes),
            f'hip_fused_{n}': (lambda: hip_drop(sk=skips), 8 + 4 * n)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--window-ms', type=float, default=400.0)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--batch', type=int, default=BATCH)
    ap.add_argument('--frames', type=int, default=FRAMES)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    benchlib.need_device('bench_dropout.py')
    dev = 'cuda:0'
    gen = torch.Generator().manual_seed(0)
    rows = []
    for b, c, t in op_shapes(args.batch, args.frames):
        ld = hip.round_up4(t)
        x = torch.randn(b, c, ld, generator=gen).to(dev)
        skips = [torch.randn(b, c, ld, generator=gen).to(dev) for _ in range(3)]
        for group in (forms(x, []), forms(x, skips[:1]), forms(x, skips)):
            fns = [fn for fn, _ in group.values()]
            benchlib.warm(fns, 5)
            probe = max(benchlib.window(fn, 20) for fn in fns)                       # ms per call of the slowest form
            calls = max(20, math.ceil(args.window_ms / probe))
            times = benchlib.alternate(fns, calls, args.reps, warmup=2)
            for (name, (_, per_element)), ts in zip(group.items(), times):
                row = {'form': name, 'batch': b, 'channels': c, 'frames': t, 'p': P, 'calls_per_window': calls, **benchlib.summary(ts, 'us', scale=1e3)}
                row['bytes'] = per_element * b * c * t
                row['gb_per_s'] = round(row['bytes'] / row['us'] / 1e3, 1)
                benchlib.emit(rows, row)
    benchlib.write_out(args.out, rows)


if __name__ == '__main__':
    main()
