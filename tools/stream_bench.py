"""Streaming inference cost (nb_asr_amd/streaming.py) on one GPU: ms per push and real-time factor at B in {1, 16, 64} and chunks of
{40, 160} input frames, the benchmark's default architecture, against the whole-utterance forward of the same 1 000 frames.

    python tools/stream_bench.py [--frames 1000] [--reps 3] [--out profiles/stream_bench.json]

A frame is 10 ms of audio (the reference's 10 ms hop): 1 000 frames = 10 s.  Real-time factor = GPU time of the session over the utterance
/ 10 s (lower is better; below 1 keeps up with live audio).  Streamed / whole = GPU time of every push + the flush over one model(x).
One JSON line per configuration; with --out also the list as a JSON file."""
import argparse
import json
import pathlib
import sys
import time

REPO = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

import torch                                     # noqa: E402

import nb_asr_amd as nb                          # noqa: E402
from nb_asr_amd.weights import keyed_fill_, keyed_input   # noqa: E402

ARCH = [[1, 0], [1, 0, 0], [1, 0, 0, 0]]        # bench.py's default architecture


def timed(fn, reps):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=1000)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--batches', default='1,16,64')
    ap.add_argument('--chunks', default='40,160')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    dev = 'cuda:0'
    model = nb.get_model(ARCH, use_rnn=True, dropout_rate=0.0)
    keyed_fill_(model, seed=1235, mode='lively')
    model = model.to(dev).eval()
    rows = []
    with torch.no_grad():
        for b in (int(v) for v in args.batches.split(',')):
            x = keyed_input(b, args.frames, seed=0).to(dev)
            model(x)                                                            # warm the whole forward (tapes, packed weights)
            model(x)
            whole_ms = timed(lambda: model(x), args.reps)
            for chunk in (int(v) for v in args.chunks.split(',')):
                sess = model.stream(batch=b, max_chunk=chunk)
                pieces = [x[:, :, i:i + chunk].contiguous() for i in range(0, args.frames, chunk)]

                def run():
                    sess.reset()
                    for p in pieces:
                        sess.push(p)
                    sess.flush()
                run()                                                           # warm-up (cached recurrence chains)
                ms = timed(run, args.reps)
                pushes = len(pieces) + 1
                row = {'batch': b, 'chunk': chunk, 'frames': args.frames, 'pushes': pushes, 'ms_per_push': round(ms / pushes, 3),
                       'stream_ms': round(ms, 2), 'whole_ms': round(whole_ms, 2), 'streamed_over_whole': round(ms / whole_ms, 2),
                       'rtf': round(ms / (args.frames * 10.0), 4), 'lookahead_frames': sess.lookahead_frames,
                       'session_mib': round(sess.buffer_bytes / 2**20, 1)}
                print(json.dumps(row), flush=True)
                rows.append(row)
                del sess
    if args.out:
        pathlib.Path(args.out).write_text(json.dumps(rows, indent=1) + '\n')


if __name__ == '__main__':
    main()
