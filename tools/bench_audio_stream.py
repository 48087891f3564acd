"""Cost of streaming from the waveform (frontend.FrontendStream, StreamingSession.push_audio) on one GPU, for B in {1, 16, 64} and pushes of
40 and 160 frames' worth of samples (6 400 / 25 600):

  (a) us per FrontendStream.push -- the fused launch of nbasr_frontend_stream_step;
  (b) us per LogMelFrontend.__call__ on a waveform with the same number of frames -- the five-launch whole-utterance chain, the baseline
      (it pads at its own ends: not usable chunk by chunk, only its cost is comparable);
  (c) ms per StreamingSession.push_audio against ms per push of ready-made features on a session of the same shape.

    python tools/bench_audio_stream.py [--pushes 50] [--reps 7] [--out profiles/streaming/audio_stream_bench.json]

Every figure is device time between two HIP events around ``--pushes`` consecutive calls (so launch gaps count, as they do for a user),
after a warm-up pass over the same shapes; the median of ``--reps`` such windows, with the smallest and largest next to it.  (a) and (b),
and the two sides of (c), alternate window by window.  One JSON line per configuration; with --out also the list as a JSON file."""
import argparse
import pathlib
import sys

REPO = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

import numpy as np                               # noqa: E402
import torch                                     # noqa: E402

import benchlib                                  # noqa: E402
from nb_asr_amd import frontend                  # noqa: E402

HOP = 160


def alternate(fns, reps):
    """(median, min, max) ms per function over ``reps`` windows each, the functions taking turns."""
    return [benchlib.summary(t) for t in benchlib.alternate(fns, reps=reps)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pushes', type=int, default=50)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--batches', default='1,16,64')
    ap.add_argument('--chunks', default='40,160')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    benchlib.need_device('bench_audio_stream.py')
    dev = 'cuda:0'
    fe = frontend.LogMelFrontend(device=dev)
    model = benchlib.session_model(dev)
    rng = np.random.default_rng(0)
    rows = []
    with torch.no_grad():
        for b in (int(v) for v in args.batches.split(',')):
            for chunk in (int(v) for v in args.chunks.split(',')):
                n, pushes = chunk * HOP, args.pushes
                wave = torch.from_numpy((0.3 * rng.standard_normal((b, n * pushes))).astype(np.float32)).to(dev)
                pieces = [wave[:, i * n:(i + 1) * n] for i in range(pushes)]
                # (b)'s waveform: chunk frames from the whole-utterance chain = (chunk - 1) * hop samples
                whole_in = wave[:, :(chunk - 1) * HOP].contiguous()
                assert fe.num_frames(whole_in.shape[1]) == chunk
                fs = fe.stream(b)

                def fused():
                    fs.reset()
                    for p in pieces:
                        fs.push(p)

                def chain():
                    for _ in range(pushes):
                        fe(whole_in)

                audio = model.stream(batch=b, max_chunk=chunk, frontend=fe)
                plain = model.stream(batch=b, max_chunk=chunk)
                feats = fe.stream(b).push(wave)                                     # the frames the audio session will compute
                feat_pieces = [feats[:, :, i * chunk:(i + 1) * chunk].contiguous() for i in range(feats.shape[2] // chunk)]

                def from_audio():
                    audio.reset()
                    for p in pieces:
                        audio.push_audio(p)

                def from_features():
                    plain.reset()
                    for p in feat_pieces:
                        plain.push(p)

                benchlib.warm((fused, chain, from_audio, from_features), 2)         # code objects, cached chains, allocator
                (a, a_lo, a_hi), (c, c_lo, c_hi) = alternate([fused, chain], args.reps)
                (pa, pa_lo, pa_hi), (pf, pf_lo, pf_hi) = alternate([from_audio, from_features], args.reps)
                us = lambda ms: round(ms * 1e3 / pushes, 1)
                row = {'batch': b, 'chunk_frames': chunk, 'chunk_samples': n, 'pushes_per_window': pushes, 'windows': args.reps,
                       'frontend_push_us': us(a), 'frontend_push_us_range': [us(a_lo), us(a_hi)],
                       'whole_chain_call_us': us(c), 'whole_chain_call_us_range': [us(c_lo), us(c_hi)],
                       'fused_over_chain': round(a / c, 3),
                       'push_audio_ms': round(pa / pushes, 3), 'push_audio_ms_range': [round(pa_lo / pushes, 3), round(pa_hi / pushes, 3)],
                       'push_features_ms': round(pf / len(feat_pieces), 3),
                       'push_features_ms_range': [round(pf_lo / len(feat_pieces), 3), round(pf_hi / len(feat_pieces), 3)],
                       'feature_pushes_per_window': len(feat_pieces),
                       'audio_over_features': round((pa / pushes) / (pf / len(feat_pieces)), 3),
                       'frontend_state_bytes': fs.state_bytes}
                benchlib.emit(rows, row)
                del audio, plain, fs
    benchlib.write_out(args.out, rows)


if __name__ == '__main__':
    main()
