"""Streaming inference cost (nb_asr_amd/streaming.py) on one GPU: ms per push and real-time factor at B in {1, 16, 64} and chunks of
{40, 160} input frames, the benchmark's default architecture, against the whole-utterance forward of the same 1 000 frames.

    python tools/stream_bench.py [--frames 1000] [--reps 3] [--dtype fp32|bf16] [--out profiles/stream_bench.json]

A frame is 10 ms of audio (the reference's 10 ms hop): 1 000 frames = 10 s.  Real-time factor = GPU time of the session over the utterance
/ 10 s (lower is better; below 1 keeps up with live audio).  Streamed / whole = GPU time of every push + the flush over one model(x).
One JSON line per configuration; with --out also the list as a JSON file.  ``--dtype bf16``: the model cast to bfloat16 and its
bfloat16 session (``StreamingSession(model, B, dtype=torch.bfloat16)``) against the bfloat16 whole forward; a row then also says so.
``--launches``: also ``launches_per_push``, the library launches of one full-size mid-stream push, counted on a launch tape.

    python tools/stream_bench.py --peek [--pairs 50] [--reps 7] [--out profiles/streaming/peek_bench.json] [--baseline parent.json]

``--peek``: the cost of ``StreamingSession.peek`` in mid-stream.  Per configuration four loops take turns, window by window: ``pairs``
pushes; ``pairs`` times push + ``peek()``; the same two with ``decode='beam'``.  A window is device time between two HIP events around the
loop (launch gaps count, as they do for a user), after the session has been fed past its lookahead; the median of ``--reps`` windows.
peek_ms = (push + peek window - push window) / pairs.  ``--package-root DIR`` measures the package of another checkout (one without
``peek`` gives the push-only columns); ``--baseline FILE`` copies that run's push-only columns next to this run's as ``parent_*``."""
import argparse
import json
import pathlib
import statistics
import sys

REPO = pathlib.Path(__file__).resolve().parent.parent
if '--package-root' in sys.argv:
    REPO = pathlib.Path(sys.argv[sys.argv.index('--package-root') + 1]).resolve()
sys.path.insert(0, str(REPO))

import torch                                     # noqa: E402

import benchlib                                  # noqa: E402
import nb_asr_amd as nb                          # noqa: E402
from nb_asr_amd.weights import keyed_input       # noqa: E402


def session_of(model, batch, chunk):
    """The session of ``model`` as it is stored: the bfloat16 one for a bfloat16 model."""
    from nb_asr_amd.streaming import StreamingSession
    if next(model.parameters()).dtype == torch.bfloat16:
        return StreamingSession(model, batch, chunk, dtype=torch.bfloat16)
    return model.stream(batch=batch, max_chunk=chunk)


def launches_of(call):
    """Library launches ``call`` enqueues."""
    entries = []
    nb.hip.start_tape(entries)
    try:
        call()
    finally:
        nb.hip.stop_tape()
    return len(entries)


def peek_rows(model, args):
    """One row per (batch, chunk): ms per push, per peek() and per peek(decode='beam') in mid-stream, and their ratios."""
    dev, pairs, rows = 'cuda:0', args.pairs, []
    for b in (int(v) for v in args.batches.split(',')):
        for chunk in (int(v) for v in args.chunks.split(',')):
            sess = session_of(model, b, chunk)
            lead = -(-(sess.lookahead_frames + chunk) // chunk)                  # pushes until every push emits frames
            x = keyed_input(b, (lead + pairs) * chunk, seed=0).to(dev).to(next(model.parameters()).dtype)
            pieces = [x[:, :, i * chunk:(i + 1) * chunk].contiguous() for i in range(lead + pairs)]
            can_peek = hasattr(sess, 'peek')

            def loop(decode, peek):
                def fn():
                    for p in pieces[lead:]:
                        sess.push(p, decode=decode)
                        if peek:
                            sess.peek(decode=decode)

                def window():
                    sess.reset()
                    for p in pieces[:lead]:
                        sess.push(p, decode=decode)
                    assert sess.frames_out > 0
                    return benchlib.window(fn)
                return window
            loops = {'push': loop(False, False), 'push_beam': loop('beam', False)}
            if can_peek:
                loops.update({'push_peek': loop(False, True), 'push_beam_peek': loop('beam', True)})
            # a loop resets and feeds its session before its window opens, so it brings its own window; two of each warm up
            times = dict(zip(loops, benchlib.alternate(list(loops.values()), reps=args.reps, warmup=2, window=lambda w, calls: w())))
            med = {k: statistics.median(t) / pairs for k, t in times.items()}
            row = {'batch': b, 'chunk': chunk, 'pairs_per_window': pairs, 'windows': args.reps, 'lookahead_frames': sess.lookahead_frames,
                   'build_id': nb.hip.load_library().nbasr_build_id().decode(),
                   'push_ms': round(med['push'], 3), 'push_ms_range': [round(min(times['push']) / pairs, 3), round(max(times['push']) / pairs, 3)],
                   'push_beam_ms': round(med['push_beam'], 3)}
            if can_peek:
                peek, peek_beam = med['push_peek'] - med['push'], med['push_beam_peek'] - med['push_beam']
                row.update({'push_peek_ms': round(med['push_peek'], 3), 'push_beam_peek_ms': round(med['push_beam_peek'], 3),
                            'peek_ms': round(peek, 3), 'peek_beam_ms': round(peek_beam, 3),
                            'peek_over_push': round(peek / med['push'], 2), 'peek_beam_over_push_beam': round(peek_beam / med['push_beam'], 2),
                            'provisional_frames': int(sess.peek().shape[1]), 'session_mib': round(sess.buffer_bytes / 2**20, 1)})
            benchlib.emit(rows, row)
            del sess
    if args.baseline:
        base = {(r['batch'], r['chunk']): r for r in json.loads(pathlib.Path(args.baseline).read_text())}
        for r in rows:
            p = base.get((r['batch'], r['chunk']))
            if p:
                r.update({'parent_build_id': p['build_id'], 'parent_push_ms': p['push_ms'], 'parent_push_ms_range': p['push_ms_range'],
                          'parent_push_beam_ms': p['push_beam_ms'], 'push_over_parent': round(r['push_ms'] / p['push_ms'], 3)})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--peek', action='store_true')
    ap.add_argument('--pairs', type=int, default=50)
    ap.add_argument('--package-root', default=None)
    ap.add_argument('--baseline', default=None)
    ap.add_argument('--frames', type=int, default=1000)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--batches', default='1,16,64')
    ap.add_argument('--chunks', default='40,160')
    ap.add_argument('--dtype', choices=('fp32', 'bf16'), default='fp32')
    ap.add_argument('--launches', action='store_true')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    benchlib.need_device('stream_bench.py')
    dev = 'cuda:0'
    model = benchlib.session_model(dev)
    if args.dtype == 'bf16':
        model = model.to(torch.bfloat16)
    rows = []
    if args.peek:
        if '--reps' not in sys.argv:
            args.reps = 7
        with torch.no_grad():
            rows = peek_rows(model, args)
    with torch.no_grad():
        for b in (int(v) for v in args.batches.split(',') if not args.peek):
            x = keyed_input(b, args.frames, seed=0).to(dev).to(next(model.parameters()).dtype)
            model(x)                                                            # warm the whole forward (tapes, packed weights)
            model(x)
            whole_ms = benchlib.best_wall_ms(lambda: model(x), args.reps)
            for chunk in (int(v) for v in args.chunks.split(',')):
                sess = session_of(model, b, chunk)
                pieces = [x[:, :, i:i + chunk].contiguous() for i in range(0, args.frames, chunk)]

                def run():
                    sess.reset()
                    for p in pieces:
                        sess.push(p)
                    sess.flush()
                run()                                                           # warm-up (cached recurrence chains)
                ms = benchlib.best_wall_ms(run, args.reps)
                pushes = len(pieces) + 1
                row = {'batch': b, 'chunk': chunk, 'frames': args.frames, 'pushes': pushes, 'ms_per_push': round(ms / pushes, 3),
                       'stream_ms': round(ms, 2), 'whole_ms': round(whole_ms, 2), 'streamed_over_whole': round(ms / whole_ms, 2),
                       'rtf': round(ms / (args.frames * 10.0), 4), 'lookahead_frames': sess.lookahead_frames,
                       'session_mib': round(sess.buffer_bytes / 2**20, 1)}
                if args.dtype != 'fp32':
                    row['dtype'] = args.dtype
                if args.launches:                                               # a full-size push in mid-stream, every stage at work
                    sess.reset()
                    for p in pieces[:-2]:
                        sess.push(p)
                    row['launches_per_push'] = launches_of(lambda: sess.push(pieces[-2]))
                benchlib.emit(rows, row)
                del sess
    benchlib.write_out(args.out, rows)


if __name__ == '__main__':
    main()
