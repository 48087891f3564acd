"""Stand-alone timing of the forward's smaller passes at the benchmark's shapes (batch 64, fp32):

    split     nbasr_layernorm_split_image at the three block boundaries (600 x 1000, 800 x 1000, 1000 x 500): the call (zero + statistics
              + normalise-and-split) and, by bytes, its rate: x read twice (the second read L2 / Infinity-Cache warm at best), the
              image (as large as x) written once
    finalize  nbasr_grouped_stats_finalize, 100 per-group partials of a 64 x 1000 tensor (51 MB)
    proj      the LSTM input projection (1200 channels x 250 frames -> 2000 gates): image passes + pw_gemm_kernel; issued 16-bit MFMA
              flops = 3 x 2 x (row tiles x 128) x (frame tiles x 256) x (K-steps x 32) per utterance

Every measurement rotates over enough buffer sets to exceed the 256 MiB last-level cache, so no call finds its operands cached by
the call before it.  Per-kernel times: run the script under `rocprofv3 --kernel-trace --stats`.

    python tools/ubench/pw_ln_passes.py [--lib OTHER/libnbasr_hip.so] [--reps 20] [--only split,finalize,proj] [--shape 600x1000]

--lib times another build of the library (a parent checkout's) in the same process layout, for A/B runs on one machine.
"""
import argparse
import pathlib
import sys

import torch

REPO = pathlib.Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(REPO))
from nb_asr_amd import hip                              # noqa: E402

DEV = 'cuda:0'
BATCH = 64
LLC = 256 << 20


def timed(calls, reps):
    """Mean microseconds per call: `calls` (one closure per buffer set) taken in turn, `reps` rounds after one warm-up round."""
    for f in calls:
        f()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        for f in calls:
            f()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / (reps * len(calls))


def sets_for(nbytes):
    return max(2, -(-2 * LLC // nbytes))


SPLIT_SHAPES = ((600, 1000), (800, 1000), (1000, 500))


def bench_split(reps, shapes=SPLIT_SHAPES):
    for c, t in shapes:
        ld = hip.row_pitch(t)
        nbytes = BATCH * c * ld * 4
        calls = []
        for _ in range(sets_for(2 * nbytes)):
            x = torch.randn(BATCH, c, ld, device=DEV)
            x[:, :, t:] = 0
            g, be = torch.rand(c, device=DEV) + 0.5, torch.randn(c, device=DEV) * 0.2
            stats, bound = torch.empty(BATCH, 2, ld, device=DEV), torch.empty(BATCH, device=DEV)
            image = hip.split_image(BATCH, c, ld, DEV)
            calls.append(lambda x=x, g=g, be=be, stats=stats, bound=bound, image=image: hip.layernorm_split_image(x, g, be, stats, bound, image, t, 1e-3))
        us = timed(calls, reps)
        print(f'split     {c:4d} x {t:4d}: {us:8.1f} us per call  ({3 * nbytes / us / 1e6:5.2f} TB/s over 2 reads + 1 write of {nbytes / 1e6:.0f} MB)', flush=True)


def bench_finalize(reps):
    c, t, groups = 1000, 1000, 100
    ld = hip.row_pitch(t)
    calls = []
    n = hip.load_library().nbasr_grouped_stats_workspace_bytes(BATCH, ld, groups) // 4
    floats = groups * BATCH * 2 * ld                    # one partial per group
    for _ in range(sets_for(floats * 4)):
        part = torch.rand(max(n, floats), device=DEV)
        out = torch.empty(BATCH, 2, ld, device=DEV)
        calls.append(lambda part=part, out=out: hip.grouped_stats_finalize(part, out, c, t, groups, 1e-3, groups_per_part=1))
    us = timed(calls, reps)
    print(f'finalize  {groups} partials, 64 x {t}: {us:8.1f} us per call  ({floats * 4 / us / 1e6:5.2f} TB/s over {floats * 4 / 1e6:.0f} MB)', flush=True)


def bench_proj(reps):
    c_in, t, hidden = 1200, 250, 500
    ld = hip.row_pitch(t)
    w = torch.randn(4 * hidden, c_in, device=DEV) * 0.03
    packed = hip.pack_pointwise_weights(w)
    b_ih, b_hh = torch.randn(4 * hidden, device=DEV), torch.randn(4 * hidden, device=DEV)
    calls = []
    for _ in range(4):                                  # x 77 MB + image 78 MB + gates 128 MB per set
        x = torch.randn(BATCH, c_in, ld, device=DEV)
        x[:, :, t:] = 0
        stats = torch.zeros(BATCH, 2, ld, device=DEV)
        ln = (hip.channel_stats(x, stats, t, 1e-3), torch.rand(c_in, device=DEV) + 0.5, torch.randn(c_in, device=DEV) * 0.2)
        ws = hip.pointwise_workspace(BATCH, c_in, ld, DEV)
        gates = torch.empty(t, BATCH, 4 * hidden, device=DEV)
        calls.append(lambda x=x, ln=ln, ws=ws, gates=gates: hip.lstm_input_projection_packed(x, t, packed, b_ih, b_hh, gates, hidden, ws, ln=ln))
    us = timed(calls, reps)
    n_mt, n_nt, n_ks = -(-4 * hidden // 128), -(-ld // 256), -(-c_in // 32)
    flops = 3 * 2 * (n_mt * 128) * (n_nt * 256) * (n_ks * 32) * BATCH
    print(f'proj      {c_in} x {t} -> {4 * hidden}: {us:8.1f} us per call (image passes + GEMM; GEMM alone: see the kernel trace); '
          f'{flops / 1e9:.1f} issued GF -> {flops / us / 1e6:.0f} TF/s if the call were the GEMM alone', flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--lib', default=None)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--only', default='split,finalize,proj')
    ap.add_argument('--shape', default=None, help="split: one shape only, as CHANNELSxFRAMES (a kernel trace then holds that shape's kernels alone)")
    args = ap.parse_args()
    if args.lib:
        hip._lib = hip.load_library(args.lib)
    print(f'library: {args.lib or hip.LIB_PATH}  build {hip.build_id()}', flush=True)
    shapes = SPLIT_SHAPES if args.shape is None else (tuple(int(v) for v in args.shape.split('x')),)
    for name in args.only.split(','):
        {'split': lambda reps: bench_split(reps, shapes), 'finalize': bench_finalize, 'proj': bench_proj}[name](args.reps)


if __name__ == '__main__':
    main()
