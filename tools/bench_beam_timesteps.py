#!/usr/bin/env python3
"""What the per-token time steps cost (ctc.beam_decode(return_timesteps=True), nbasr_ctc_beam_search_timed) at the bench shape: B = 64
utterances of 250 output frames, 49 classes, width 12 -- the timed search against the untimed one, and the untimed one against the same
entry point of another build of the library (the parent commit's: the untimed path must not pay for the timed one).

    python tools/bench_beam_timesteps.py [--other-lib path/to/libnbasr_hip.so] [--iters 30] [--out profiles/streaming/beam_timesteps_bench.json]

GPU time from device events around one call (pruning pre-pass + search), median over --iters calls after warm-up; the variants are timed
in alternation, round by round, so that a drift of the machine falls on all of them.  Both libraries are driven through the C ABI with
the same preallocated buffers; the results of the two untimed searches are compared bit for bit, and the timed one's beams with them."""
import argparse
import ctypes
import pathlib
import statistics
import sys

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


class Search:
    """One library's whole-utterance search over fixed buffers: ``run()`` enqueues it, ``result()`` gives its outputs."""

    def __init__(self, lib, lp, width, timed):
        b, t, c = lp.shape
        self.lib, self.lp, self.timed, self.dims = lib, lp, timed, (b, t, c, width, 0, 40)
        dev = lp.device
        self.beams = torch.empty(b, width, t, dtype=torch.int32, device=dev)
        self.steps = torch.empty(b, width, t, dtype=torch.int32, device=dev)
        self.scores = torch.empty(b, width, dtype=torch.float32, device=dev)
        self.lens = torch.empty(b, width, dtype=torch.int32, device=dev)
        size = lib.nbasr_ctc_beam_timed_workspace_bytes if timed else lib.nbasr_ctc_beam_workspace_bytes
        size.restype, size.argtypes = ctypes.c_size_t, [ctypes.c_int] * 4
        self.ws = torch.empty(size(b, t, c, width) // 8 + 1, dtype=torch.int64, device=dev)
        self.fn = lib.nbasr_ctc_beam_search_timed if timed else lib.nbasr_ctc_beam_search
        self.fn.restype = ctypes.c_int
        self.fn.argtypes = [ctypes.c_void_p] * (7 if timed else 6) + [ctypes.c_int] * 6 + [ctypes.c_void_p]
        self.stream = torch.cuda.current_stream(dev).cuda_stream

    def run(self):
        outs = [self.beams, self.scores] + ([self.steps] if self.timed else []) + [self.lens]
        rc = self.fn(self.lp.data_ptr(), None, self.ws.data_ptr(), *(o.data_ptr() for o in outs), *self.dims, self.stream)
        if rc != 0:
            raise SystemExit(f'search failed with {rc}')

    def result(self):
        self.run()
        torch.cuda.synchronize()
        return self.beams.clone(), self.scores.clone(), self.lens.clone()


def alternate(variants, iters, warmup=5):
    """{name: median GPU ms} of the variants' ``run``, one call of each per round."""
    rounds = benchlib.alternate([v.run for v in variants.values()], reps=warmup + iters)
    times = {name: t[warmup:] for name, t in zip(variants, rounds)}
    return {name: statistics.median(t) for name, t in times.items()}, {name: (min(t), max(t)) for name, t in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--frames', type=int, default=250)
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--other-lib', default=None, help='another build of libnbasr_hip.so whose untimed search is timed alongside')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    this = ctypes.CDLL(str(hip.LIB_PATH))
    other = ctypes.CDLL(a.other_lib) if a.other_lib else None
    rows = []
    for sharp, name in ((1.0, 'flat'), (6.0, 'peaked')):
        lp = inputs(a.batch, a.frames, sharp)
        variants = {'untimed': Search(this, lp, 12, False), 'timed': Search(this, lp, 12, True)}
        if other is not None:
            variants['other_untimed'] = Search(other, lp, 12, False)
        want = variants['untimed'].result()
        for v in variants.values():
            if not all(torch.equal(g, w) for g, w in zip(v.result(), want)):
                raise SystemExit('the searches disagree')
        med, spread = alternate(variants, a.iters)
        row = {'input': name, 'batch': a.batch, 'frames': a.frames, 'width': 12, 'iters': a.iters,
               'untimed_us': round(med['untimed'] * 1e3, 1), 'timed_us': round(med['timed'] * 1e3, 1),
               'timed_vs_untimed': round(med['timed'] / med['untimed'], 4),
               'min_max_us': {k: [round(lo * 1e3, 1), round(hi * 1e3, 1)] for k, (lo, hi) in spread.items()}}
        if other is not None:
            row['other_untimed_us'] = round(med['other_untimed'] * 1e3, 1)
            row['untimed_vs_other'] = round(med['untimed'] / med['other_untimed'], 4)
        benchlib.emit(rows, row)
    write_out(a.out, rows, other)


def write_out(path, rows, other):
    """The rows under this build's id and the device's name, and the other library's id where there is one."""
    out = {'build_id': hip.build_id(), 'device': torch.cuda.get_device_name(0), 'rows': rows}
    if other is not None:
        other.nbasr_build_id.restype = ctypes.c_char_p
        out['other_build_id'] = other.nbasr_build_id().decode()
    benchlib.write_out(path, out)


if __name__ == '__main__':
    main()
