"""Cost of the HIP resampler (frontend.Resampler / ResamplerStream, nbasr_resample*) on one GPU, to 16 kHz from 8, 11.025, 44.1 and 48 kHz:

  (a) us per ResamplerStream.push for B in {1, 16, 64} and pushes of 0.4 s of audio (the samples of 40 frames) -- one launch, plus
      the allocation of its output;
  (b) us per Resampler.__call__ on B = 64 utterances of 10 s, with the bytes it must move (samples in, outputs out) over that time.

    python tools/bench_resample.py [--pushes 50] [--reps 7] [--out profiles/streaming/resample_bench.json]

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
from nb_asr_amd import frontend                  # noqa: E402

RATES = (8000, 11025, 44100, 48000)


def timed(fn, calls, reps):
    (times,) = benchlib.alternate([fn], calls, reps, warmup=1)
    return benchlib.summary(times, 'us', scale=1e3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pushes', type=int, default=50)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--batches', default='1,16,64')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    benchlib.need_device('bench_resample.py')
    dev = 'cuda:0'
    gen = torch.Generator().manual_seed(0)
    rows = []
    for rate in RATES:
        r = frontend.Resampler(rate, 16000, device=dev)
        for b in (int(v) for v in args.batches.split(',')):
            chunk = torch.randn(b, rate * 2 // 5, generator=gen).to(dev)
            rs = r.stream(b)
            benchlib.emit(rows, {'what': 'ResamplerStream.push', 'rate': rate, 'batch': b, 'samples_per_push': chunk.shape[1],
                                 **timed(lambda: rs.push(chunk), args.pushes, args.reps)})
        wave = torch.randn(64, 10 * rate, generator=gen).to(dev)
        row = {'what': 'Resampler.__call__', 'rate': rate, 'batch': 64, 'samples': wave.shape[1], **timed(lambda: r(wave), args.pushes, args.reps)}
        row['bytes'] = 4 * 64 * (wave.shape[1] + r.out_len(wave.shape[1]))
        row['gb_per_s'] = round(row['bytes'] / row['us'] / 1e3, 1)
        benchlib.emit(rows, row)
    benchlib.write_out(args.out, rows)


if __name__ == '__main__':
    main()
