#!/usr/bin/env python3
"""What bigram LM fusion costs (ctc.beam_decode(lm=...), nbasr_ctc_beam_search_lm / nbasr_ctc_beam_stream_lm_step) at the shapes
tools/bench_decode.py uses: B = 64 utterances of 250 output frames, 49 classes, width 12, flat and peaked inputs -- the fused search against
the unfused one, the fused stream step against the unfused one in chunks of 10 and 40 frames, and the unfused ones against the same entry
points of another build of the library (the parent commit's: the unfused path must not pay for the fused one).

    python tools/bench_beam_lm.py [--other-lib path/to/libnbasr_hip.so] [--iters 30] [--out profiles/decode/lm_fusion_bench.json]

GPU time from device events around one call (pruning pre-pass + search), or around the init and all steps of one stream over the 250 frames
(no read-back between the steps: the pool is sized so that no step can be refused); median over --iters rounds after warm-up, the variants
timed in alternation, round by round, so that a drift of the machine falls on all of them.  Everything is driven through the C ABI over
preallocated buffers.  The two unfused searches are compared bit for bit, and so is the fused one with an all-zero table -- which is also
timed (fused_zero): it walks exactly the unfused search's beams, so its ratio is the cost of the mechanism alone, while a real table also
changes which prefixes live, merge and get rescanned."""
import argparse
import ctypes
import pathlib
import sys

REPO = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

import torch                                     # noqa: E402

import benchlib                                  # noqa: E402
from bench_beam_timesteps import Search, alternate, inputs, write_out      # noqa: E402
from nb_asr_amd import hip                       # noqa: E402

P, I = ctypes.c_void_p, ctypes.c_int


class FusedSearch(Search):
    """``Search`` through nbasr_ctc_beam_search_lm with the table ``fusion`` (untimed)."""

    def __init__(self, lib, lp, width, fusion):
        super().__init__(lib, lp, width, False)
        self.fusion = fusion
        self.fn = lib.nbasr_ctc_beam_search_lm
        self.fn.restype, self.fn.argtypes = I, [P] * 8 + [I] * 7 + [P]

    def run(self):
        rc = self.fn(self.lp.data_ptr(), None, self.fusion.data_ptr(), self.ws.data_ptr(), self.beams.data_ptr(), self.scores.data_ptr(), None,
                     self.lens.data_ptr(), *self.dims, 0, self.stream)
        if rc != 0:
            raise SystemExit(f'fused search failed with {rc}')


class Stream:
    """One library's streaming search over ``lp`` in chunks of ``push`` frames: ``run()`` enqueues the init and every step."""

    def __init__(self, lib, lp, width, push, fusion=None):
        b, t, c = lp.shape
        dev = lp.device
        self.lib, self.fusion, self.b, self.c, self.width = lib, fusion, b, c, width
        self.pool = 2 + width * (t + push + 1)               # usage <= 1 + width * t: no step is ever refused
        self.chunks = [lp[:, at:at + push].contiguous() for at in range(0, t, push)]
        for fn, ret, args in ((lib.nbasr_ctc_beam_stream_state_bytes, ctypes.c_size_t, [I] * 3),
                              (lib.nbasr_ctc_beam_stream_workspace_bytes, ctypes.c_size_t, [I] * 4),
                              (lib.nbasr_ctc_beam_stream_init, I, [P] + [I] * 3 + [P]),
                              (lib.nbasr_ctc_beam_stream_step, I, [P] * 9 + [I] * 7 + [P]),
                              (lib.nbasr_ctc_beam_stream_finish, I, [P] * 4 + [I] * 4 + [P])):
            fn.restype, fn.argtypes = ret, args
        if fusion is not None:
            lib.nbasr_ctc_beam_stream_lm_step.restype, lib.nbasr_ctc_beam_stream_lm_step.argtypes = I, [P] * 12 + [I] * 8 + [P]
        self.state = torch.empty(lib.nbasr_ctc_beam_stream_state_bytes(b, width, self.pool) // 8 + 1, dtype=torch.int64, device=dev)
        self.ws = torch.empty(lib.nbasr_ctc_beam_stream_workspace_bytes(b, push, c, self.pool) // 8 + 1, dtype=torch.int64, device=dev)
        self.rows = torch.empty(2, b, self.pool, dtype=torch.int32, device=dev)
        self.counts = torch.empty(3, b, dtype=torch.int32, device=dev)
        self.beams = torch.empty(b, width, t, dtype=torch.int32, device=dev)
        self.scores = torch.empty(b, width, dtype=torch.float32, device=dev)
        self.lens = torch.empty(b, width, dtype=torch.int32, device=dev)
        self.stream = torch.cuda.current_stream(dev).cuda_stream

    def run(self):
        lib, b, w = self.lib, self.b, self.width
        rc = lib.nbasr_ctc_beam_stream_init(self.state.data_ptr(), b, w, self.pool, self.stream)
        for chunk in self.chunks:
            outs = (self.rows[0].data_ptr(), self.counts[0].data_ptr(), self.rows[1].data_ptr(), self.counts[1].data_ptr(), self.counts[2].data_ptr())
            dims = (b, chunk.shape[1], self.c, w, 0, 40, self.pool)
            if self.fusion is None:
                rc |= lib.nbasr_ctc_beam_stream_step(chunk.data_ptr(), None, self.state.data_ptr(), self.ws.data_ptr(), *outs, *dims, self.stream)
            else:
                rc |= lib.nbasr_ctc_beam_stream_lm_step(chunk.data_ptr(), None, self.fusion.data_ptr(), self.state.data_ptr(), self.ws.data_ptr(),
                                                        outs[0], None, outs[1], outs[2], None, outs[3], outs[4], *dims, 0, self.stream)
        if rc != 0:
            raise SystemExit(f'stream failed with {rc}')

    def result(self):
        """The live suffixes after the last step (the committed heads are not assembled: equal states give equal suffixes)."""
        self.run()
        rc = self.lib.nbasr_ctc_beam_stream_finish(self.state.data_ptr(), self.beams.data_ptr(), self.scores.data_ptr(), self.lens.data_ptr(),
                                                   self.beams.shape[2], self.b, self.width, self.pool, self.stream)
        torch.cuda.synchronize()
        if rc != 0 or int(self.counts[2].min()) < 0:
            raise SystemExit('stream finish failed, or a step was refused')
        return self.beams.clone(), self.scores.clone(), self.lens.clone()


def same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def timed_row(variants, iters, base='unfused'):
    med, spread = alternate(variants, iters)
    row = {f'{name}_us': round(ms * 1e3, 1) for name, ms in med.items()}
    row['fused_vs_unfused'] = round(med['fused'] / med[base], 4)
    row['fused_zero_vs_unfused'] = round(med['fused_zero'] / med[base], 4)
    if 'other_unfused' in med:
        row['unfused_vs_other'] = round(med[base] / med['other_unfused'], 4)
    row['min_max_us'] = {k: [round(lo * 1e3, 1), round(hi * 1e3, 1)] for k, (lo, hi) in spread.items()}
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--frames', type=int, default=250)
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--pushes', type=int, nargs='+', default=[10, 40])
    ap.add_argument('--other-lib', default=None, help='another build of libnbasr_hip.so whose unfused entry points are timed alongside')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    this = ctypes.CDLL(str(hip.LIB_PATH))
    other = ctypes.CDLL(a.other_lib) if a.other_lib else None
    gen = torch.Generator().manual_seed(1)
    table = (torch.randn(49, 49, generator=gen) - 3.0).to('cuda:0')          # log-probability-like: negative, a few nats apart
    zero = torch.zeros(49, 49, device='cuda:0')
    rows = []
    for sharp, name in ((1.0, 'flat'), (6.0, 'peaked')):
        lp = inputs(a.batch, a.frames, sharp)
        variants = {'unfused': Search(this, lp, 12, False), 'fused': FusedSearch(this, lp, 12, table), 'fused_zero': FusedSearch(this, lp, 12, zero)}
        if other is not None:
            variants['other_unfused'] = Search(other, lp, 12, False)
        want = variants['unfused'].result()
        if not same(variants['fused_zero'].result(), want) or (other is not None and not same(variants['other_unfused'].result(), want)):
            raise SystemExit('the searches disagree')
        row = {'input': name, 'batch': a.batch, 'frames': a.frames, 'width': 12, 'iters': a.iters, 'search': timed_row(variants, a.iters),
               'fused_changes_best_beams': int((variants['fused'].result()[0][:, 0] != want[0][:, 0]).any(1).sum()), 'streams': []}
        for push in a.pushes:
            variants = {'unfused': Stream(this, lp, 12, push), 'fused': Stream(this, lp, 12, push, table), 'fused_zero': Stream(this, lp, 12, push, zero)}
            if other is not None:
                variants['other_unfused'] = Stream(other, lp, 12, push)
            want_s = variants['unfused'].result()
            if not same(variants['fused_zero'].result(), want_s) or (other is not None and not same(variants['other_unfused'].result(), want_s)):
                raise SystemExit('the streams disagree')
            row['streams'].append({'push_frames': push, 'pushes': len(variants['unfused'].chunks), **timed_row(variants, a.iters)})
        benchlib.emit(rows, row)
    write_out(a.out, rows, other)


if __name__ == '__main__':
    main()
