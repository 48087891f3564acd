"""Cost of a logit detector on one GPU -- the endpointer (ctc.endpoint / EndpointStream, nbasr_ctc_endpoint_step; StreamingSession(endpoint=)),
the keyword spotter (ctc.spot_keywords / KeywordStream, nbasr_ctc_keyword_step; StreamingSession(keywords=), 8 keywords) or the segmenter
(ctc.segment / SegmentStream, nbasr_ctc_segment_step; StreamingSession(segments=)):

  (a) us per StreamingSession.push of 40 feature frames (10 logit frames a push) at B in {1, 16}, with and without the detector, the two
      sessions alternating window by window -- and, with --parent-library, the same push without it on another build of the library
      (the parent commit's), measured by a child process of this tool before and after the windows of this one; then this library's
      plain push over the mean of the parent's two legs, with the parent's own leg-to-leg ratio beside it;
  (b) endpoint, segment: us per ctc.endpoint / ctc.segment on (64, 250, 49) logits, with the bytes it reads over that time;
  (c) us per <Detector>Stream.push -- the step alone -- at B in {1, 16}: endpoint and segment at 1, 10 and 40 frames, keyword at
      {1, 8, 64} keywords x {4, 250} frames.  For the segmenter EndpointStream.push takes turns with it, window by window, at every
      shape (it has the endpointer's launch shape: same process, same library), and the ratio of the two is a row.

    python tools/bench_detector.py --detector endpoint|keyword|segment [--pushes 50] [--reps 7] [--batches 1,16] [--parent-library PATH]
                                   [--out profiles/streaming/<detector>_bench.json]

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
from nb_asr_amd import ctc, streaming            # noqa: E402

CHUNK = 40                                       # feature frames a push: 0.4 s of audio, 10 logit frames
SESSION_KEYWORDS = 8
WARMUP = 2                                       # calls of each function before its windows


def keyword_set(count, dev, seed=0):
    """``count`` keywords of 2 to 12 phonemes (one of them of 32), the default (untuned) thresholds."""
    gen = torch.Generator().manual_seed(seed)
    words = [torch.randint(1, 49, (int(torch.randint(2, 13, (1,), generator=gen)),), generator=gen).tolist() for _ in range(count)]
    words[-1] = torch.randint(1, 49, (32,), generator=gen).tolist()
    return ctc.KeywordSet(words, device=dev)


# Per detector: the session's keyword argument (also the noun of the labels) and what builds its spec on ``dev``; keys that the 'added
# by' row carries; the stream class; the whole-utterance call, if it is measured; the grid of the step alone -- (extra row keys, spec on
# ``dev``, frames per push) -- and the detector whose step takes turns with this one, if any.
def endpoint_rules(dev):
    return ctc.EndpointRules(device=dev)


def segment_rules(dev):
    return ctc.SegmentRules(device=dev)


DETECTORS = {
    'endpoint': dict(kwarg='endpoint', spec=endpoint_rules, added={}, stream=ctc.EndpointStream, whole=ctc.endpoint,
                     grid=[({}, endpoint_rules, (1, 10, 40))], beside=None),
    'keyword': dict(kwarg='keywords', spec=lambda dev: keyword_set(SESSION_KEYWORDS, dev), added={'keywords': SESSION_KEYWORDS},
                    stream=ctc.KeywordStream, whole=None,
                    grid=[({'keywords': n}, lambda dev, n=n: keyword_set(n, dev, seed=n), (4, 250)) for n in (1, 8, 64)], beside=None),
    'segment': dict(kwarg='segments', spec=segment_rules, added={}, stream=ctc.SegmentStream, whole=ctc.segment,
                    grid=[({}, segment_rules, (1, 10, 40))], beside='endpoint'),
}


def measure(fns, args):
    """One {'us', 'us_min', 'us_max'} per function, the functions taking turns."""
    return [benchlib.summary(t, 'us', scale=1e3) for t in benchlib.alternate(fns, args.pushes, args.reps, warmup=WARMUP)]


def session_rows(det, args, batches, library, with_detector):
    """(a): the push of a session in steady state (it has emitted frames: every push commits 10 more)."""
    dev, kwarg = 'cuda:0', det['kwarg']
    model = benchlib.session_model(dev)
    rows = []
    with torch.no_grad():
        for b in batches:
            chunk = torch.randn(b, streaming.FEATURES, CHUNK, generator=torch.Generator().manual_seed(b)).to(dev)
            kinds = [(f'without {kwarg}=', {})] + ([(f'with {kwarg}=', {kwarg: det['spec'](dev)})] if with_detector else [])
            sessions = [streaming.StreamingSession(model, b, max_chunk=CHUNK, **kw) for _, kw in kinds]
            for s in sessions:                   # past the lookahead
                for _ in range(s.lookahead_frames // CHUNK + 2):
                    s.push(chunk)
            results = measure([lambda s=s: s.push(chunk) for s in sessions], args)
            for (kind, _), r in zip(kinds, results):
                benchlib.emit(rows, {'what': 'StreamingSession.push', 'session': kind, 'library': library, 'batch': b, 'frames_per_push': CHUNK, **r})
            if with_detector:
                benchlib.emit(rows, {'what': f'added by {kwarg}=', 'library': library, 'batch': b, **det['added'],
                                     'us': round(results[1]['us'] - results[0]['us'], 2), 'ratio': round(results[1]['us'] / results[0]['us'], 4)})
    return rows


def step_rows(det, args, batches, gen):
    """(c): the step alone, beside the ``beside`` detector's where there is one."""
    dev, rows = 'cuda:0', []
    beside = DETECTORS[det['beside']] if det['beside'] else None
    for b in batches:
        for extra, spec, frames in det['grid']:
            for n in frames:
                chunk = torch.randn(b, n, 49, generator=gen).to(dev)
                streams = ([beside['stream'](b, beside['spec'](dev), dev)] if beside else []) + [det['stream'](b, spec(dev), dev)]
                results = measure([lambda s=s: s.push(chunk) for s in streams], args)
                for s, r in zip(streams, results):
                    benchlib.emit(rows, {'what': f'{type(s).__name__}.push', 'batch': b, **extra, 'frames': n, **r})
                if len(streams) == 2:
                    names = [type(s).__name__ for s in streams]
                    benchlib.emit(rows, {'what': f'{names[1]}.push over {names[0]}.push', 'batch': b, 'frames': n,
                                         'ratio': round(results[1]['us'] / results[0]['us'], 4)})
    return rows


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--detector', required=True, choices=sorted(DETECTORS))
    ap.add_argument('--pushes', type=int, default=50)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--batches', default='1,16')
    ap.add_argument('--parent-library', default=None, help='another libnbasr_hip.so to measure the plain push on (the parent commit\'s)')
    ap.add_argument('--library', default=None, help='measure ONLY the plain push, on this library (what --parent-library starts)')
    ap.add_argument('--out', default=None)
    args = ap.parse_args(argv)
    benchlib.need_device('bench_detector.py')
    det = DETECTORS[args.detector]
    batches = [int(v) for v in args.batches.split(',')]
    if args.library:                             # an older build: bind what it exports, measure what it can do
        benchlib.bind_library(args.library)
        return session_rows(det, args, batches, args.library, with_detector=False)
    dev = 'cuda:0'
    child = ['--detector', args.detector, '--pushes', str(args.pushes), '--reps', str(args.reps), '--batches', args.batches]
    rows = benchlib.parent_rows(__file__, args.parent_library, 'before', child) if args.parent_library else []
    rows += session_rows(det, args, batches, 'this', with_detector=True)
    if args.parent_library:
        rows += benchlib.parent_rows(__file__, args.parent_library, 'after', child)
        for row in benchlib.parent_ratio_rows(rows, batches, f'without {det["kwarg"]}='):
            benchlib.emit(rows, row)
    gen = torch.Generator().manual_seed(0)
    if det['whole']:                             # (b) whole utterances
        x, spec = torch.randn(64, 250, 49, generator=gen).to(dev), det['spec'](dev)
        (r,) = measure([lambda: det['whole'](x, None, spec)], args)
        row = {'what': f'ctc.{det["whole"].__name__}', 'shape': list(x.shape), **r, 'bytes': x.numel() * 4}
        row['gb_per_s'] = round(row['bytes'] / row['us'] / 1e3, 1)
        benchlib.emit(rows, row)
    rows += step_rows(det, args, batches, gen)
    benchlib.write_out(args.out, rows)
    return rows


if __name__ == '__main__':
    main()
