#!/usr/bin/env python3
"""Streaming beam decode cost (ctc.BeamSearchStream, nbasr_ctc_beam_stream_*) at the bench shape: B = 64 utterances of 250 output frames,
49 classes, width 12, against one ctc.beam_decode of the same 250 frames.

    python tools/bench_beam_stream.py [--batch 64] [--frames 250] [--iters 10] [--out profiles/streaming/beam_stream_bench.json]

GPU time: device events around the work each entry point enqueues (for a stream: every step, pruning pre-pass included; the host
reads the counts back between steps, as BeamSearchStream does, and that gap is not counted).  Wall time: the whole BeamSearchStream
loop with its read-backs and finish().  Also: state bytes per utterance, the largest pool usage, and the committed-token lag -- for every
token of the final best beam that was committed before finish(), the frames between the push after which the best hypothesis (committed +
partial) first held that token for good and the push that committed it, measured with pushes of 1 frame and of the timed sizes."""
import argparse
import pathlib
import statistics
import sys
import time

REPO = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

import torch                                     # noqa: E402

import benchlib                                  # noqa: E402
from nb_asr_amd import ctc, hip                  # noqa: E402


def inputs(batch, frames, sharp, seed=0):
    gen = torch.Generator().manual_seed(seed)
    logits = torch.randn(batch, frames, 49, generator=gen) * sharp
    logits[:, ::2, 0] += 2.0 * sharp
    return ctc.log_softmax(logits.to('cuda:0'))


def gpu_ms(fn, iters):
    (out,) = benchlib.alternate([fn], reps=iters + 2)
    return statistics.median(out[2:])


def stream_gpu_ms(lp, push, iters, width=12):
    """Summed event time of the steps of one stream over lp in pushes of `push` frames (median over iters streams)."""
    b, t, _ = lp.shape
    pool = 1 + width * (t + 1)                           # never too small: usage, not the pool size, sets the cost
    state = torch.empty((hip.ctc_beam_stream_state_bytes(b, width, pool) + 7) // 8, dtype=torch.int64, device=lp.device)
    totals, usage_max = [], 0
    for _ in range(iters + 2):
        hip.ctc_beam_stream_init(state, b, width, pool)
        total = 0.0
        for at in range(0, t, push):
            chunk, outs = lp[:, at:at + push].contiguous(), []
            total += benchlib.window(lambda: outs.append(hip.ctc_beam_stream_step(chunk, None, state, width, pool)))
            counts = outs[0][2].cpu()                            # the host's read-back between pushes
            usage = int(counts[2].max())
            if usage < 0 or usage + width * push + 1 > pool:
                raise SystemExit(f'pool of {pool} nodes too small for this input (usage {usage})')
            usage_max = max(usage_max, usage)
        totals.append(total)
    return statistics.median(totals[2:]), usage_max, pool


def stream_wall_ms(lp, push, iters):
    b, t, _ = lp.shape
    out = []
    for _ in range(iters + 2):
        dec = ctc.BeamSearchStream(b, device=lp.device)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for at in range(0, t, push):
            dec.push(lp[:, at:at + push])
        dec.finish()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out[2:]), dec.state_bytes // b


def commit_lag(lp, push):
    """Mean and max frames between a token's settling in the best hypothesis and its commit; and the fraction committed before finish."""
    b, t, _ = lp.shape
    dec = ctc.BeamSearchStream(b, device=lp.device)
    hyps = [[] for _ in range(b)]                          # per push: (frames so far, committed count, committed + partial)
    committed = [[] for _ in range(b)]
    for at in range(0, t, push):
        new, partial = dec.push(lp[:, at:at + push])
        end = min(at + push, t)
        for i in range(b):
            committed[i] += new[i].tolist()
            hyps[i].append((end, len(committed[i]), committed[i] + partial[i].tolist()))
    beams, _, lens = (x.cpu() for x in dec.finish())
    lags, n_tokens, n_committed = [], 0, 0
    for i in range(b):
        final = beams[i, 0, : int(lens[i, 0])].tolist()
        n_tokens += len(final)
        for k in range(len(committed[i])):
            n_committed += 1
            commit_at = next(end for end, n_c, _ in hyps[i] if n_c > k)
            settled = commit_at
            for end, _, hyp in reversed([h for h in hyps[i] if h[0] <= commit_at]):
                if hyp[: k + 1] != final[: k + 1]:
                    break
                settled = end
            lags.append(commit_at - settled)
    return {'push': push, 'mean_lag_frames': round(statistics.mean(lags), 2) if lags else None, 'max_lag_frames': max(lags) if lags else None,
            'committed_before_finish': round(n_committed / max(n_tokens, 1), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--frames', type=int, default=250)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--pushes', type=int, nargs='+', default=[10, 40])
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    rows = []
    for sharp, name in ((1.0, 'flat'), (6.0, 'peaked')):
        lp = inputs(a.batch, a.frames, sharp)
        whole = gpu_ms(lambda: ctc.beam_decode(lp, None), a.iters)
        row = {'input': name, 'batch': a.batch, 'frames': a.frames, 'width': 12, 'whole_beam_decode_us': round(whole * 1e3, 1),
               'whole_us_per_frame': round(whole * 1e3 / a.frames, 2), 'streams': []}
        for push in a.pushes:
            g, usage_max, pool = stream_gpu_ms(lp, push, a.iters)
            wall, per_utt = stream_wall_ms(lp, push, max(a.iters // 2, 1))
            pushes = -(-a.frames // push)
            row['streams'].append({'push_frames': push, 'pushes': pushes, 'gpu_us': round(g * 1e3, 1), 'gpu_vs_whole': round(g / whole, 3),
                                   'gpu_overhead_us_per_push': round((g - whole) * 1e3 / pushes, 1), 'wall_us_with_readbacks': round(wall * 1e3, 1),
                                   'state_bytes_per_utterance': per_utt, 'max_pool_usage': usage_max, 'timed_pool_nodes': pool})
        row['commit_lag'] = [commit_lag(lp, p) for p in [1] + list(a.pushes)]
        benchlib.emit(rows, row)
    benchlib.write_out(a.out, {'build_id': hip.build_id(), 'device': torch.cuda.get_device_name(0), 'rows': rows})


if __name__ == '__main__':
    main()
