"""Cost of CTC forced alignment on one GPU, beside the CTC loss-and-gradient kernel at the same shape, measured in the same run:

  (a) microseconds per ``nbasr_ctc_forced_align`` (one launch: max-sweep with 2-bit back-pointers, the walk back, spans and token scores);
  (b) microseconds per ``nbasr_ctc_loss_grad`` (one launch: the alpha sweep through a global workspace, the beta sweep with the gradient rows).

    python tools/align_bench.py [--calls 500] [--reps 7] [--out profiles/align/align_bench.json]

at (64 utterances x 250 frames x 49 classes, 40 labels) and (8 x 250 x 49, 40 labels): the validation batch of the reference's trainer and a
small one.  Both entry points are called through the C ABI on buffers allocated once (outputs and workspaces included), every utterance at
its full length with 40 random labels on the log-softmax of random logits.  Every figure is device time between two HIP events around
``--calls`` consecutive launches, after a warm-up window, divided by the calls; the median of ``--reps`` such windows with the smallest and
largest next to it; (a) and (b) alternate window by window.  Recorded, not gated: no test holds a threshold against these numbers."""
import argparse
import pathlib
import sys

REPO = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

import torch                                     # noqa: E402

import benchlib                                  # noqa: E402
from nb_asr_amd import hip                       # noqa: E402

SHAPES = [(64, 250, 49, 40), (8, 250, 49, 40)]  # batch, frames, classes, labels


def measure(shape, calls, reps, dev):
    b, frames, classes, labels = shape
    lib = hip.load_library()
    gen = torch.Generator().manual_seed(b)
    log_probs = torch.log_softmax(torch.randn(b, frames, classes, generator=gen) * 2.0, dim=2).to(dev)
    targets = torch.randint(1, classes, (b, labels), generator=gen, dtype=torch.int32).to(dev)
    lengths = torch.full((b,), frames, dtype=torch.int32, device=dev)
    target_lengths = torch.full((b,), labels, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    align_ws = torch.empty(lib.nbasr_ctc_align_workspace_bytes(b, frames, labels) // 4, dtype=torch.int32, device=dev)
    scores, token_scores = torch.empty(b, device=dev), torch.empty(b, labels, device=dev)
    path = torch.empty(b, frames, dtype=torch.int32, device=dev)
    starts, ends = torch.empty(b, labels, dtype=torch.int32, device=dev), torch.empty(b, labels, dtype=torch.int32, device=dev)
    grad_ws = torch.empty(lib.nbasr_ctc_grad_workspace_bytes(b, frames, labels) // 4, device=dev)
    losses, grad = torch.empty(b, device=dev), torch.empty_like(log_probs)

    def align():
        for _ in range(calls):
            rc = lib.nbasr_ctc_forced_align(log_probs.data_ptr(), lengths.data_ptr(), targets.data_ptr(), target_lengths.data_ptr(), align_ws.data_ptr(),
                                            scores.data_ptr(), path.data_ptr(), starts.data_ptr(), ends.data_ptr(), token_scores.data_ptr(),
                                            b, frames, classes, labels, 0, stream)
            assert rc == 0, lib.nbasr_last_error()

    def loss_grad():
        for _ in range(calls):
            rc = lib.nbasr_ctc_loss_grad(log_probs.data_ptr(), lengths.data_ptr(), targets.data_ptr(), target_lengths.data_ptr(), grad_ws.data_ptr(),
                                         losses.data_ptr(), grad.data_ptr(), b, frames, classes, labels, 0, stream)
            assert rc == 0, lib.nbasr_last_error()

    benchlib.warm((align, loss_grad), 1)         # code objects, clocks
    if not bool(torch.isfinite(scores).all()) or not bool(torch.isfinite(losses).all()):
        raise SystemExit('align_bench.py: the inputs were meant to align; the figures would time the early exit')
    (a, a_lo, a_hi), (g, g_lo, g_hi) = (benchlib.summary(t) for t in benchlib.alternate([align, loss_grad], reps=reps))
    per = lambda ms: round(ms / calls * 1e3, 2)
    return {'batch': b, 'frames': frames, 'classes': classes, 'labels': labels, 'calls_per_window': calls, 'windows': reps,
            'forced_align_us': per(a), 'forced_align_us_range': [per(a_lo), per(a_hi)],
            'loss_grad_us': per(g), 'loss_grad_us_range': [per(g_lo), per(g_hi)],
            'align_over_loss_grad': round(a / g, 3), 'align_workspace_bytes': align_ws.numel() * 4, 'loss_grad_workspace_bytes': grad_ws.numel() * 4}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=500)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    benchlib.need_device('align_bench.py')
    rows = []
    for shape in SHAPES:
        benchlib.emit(rows, dict(measure(shape, args.calls, args.reps, 'cuda:0'), build_id=hip.build_id()))
    benchlib.write_out(args.out, rows)


if __name__ == '__main__':
    main()
