"""Cost of the optimisation step on one GPU, over the parameter tensors of bench.py's default architecture (166 tensors, 105 MB of fp32),
with gradients already present:

  (a) ms per ``optim.Adam.step`` in the reference's configuration (``optim.reference_optimizer``) -- three launches of nbasr_optim_adam_step;
  (b) ms per torch recipe -- the regulariser's backward into ``.grad`` (0.01 * sum(torch.norm(conv.weight))), ``clip_grad_norm_(params, 5)``
      and ``torch.optim.Adam(lr, eps=1e-7).step()`` -- on a copy of the same tensors.

    python tools/bench_optim.py [--calls 50] [--reps 7] [--out profiles/training/optim_bench.json]

Every figure is device time between two HIP events around ``--calls`` consecutive steps (so launch gaps and host work count, as they do for a
user), after a warm-up pass; the median of ``--reps`` such windows, with the smallest and largest next to it; (a) and (b) alternate window
by window.  Bytes per step are counted as 9 x the parameter bytes: the norm pass reads g, the update reads p, g, m, v and writes p, m, v
(the regulariser's second read of the flagged weights, 2 % of the set, is left out) -- the same count for both sides.
The two sides start from the same values and do not stay the same tensors: nothing zeroes ``.grad`` between the calls, so on side (b) the
regulariser's backward and the clip keep accumulating into it, while (a) only reads it.  Restoring it would add a 105 MB copy to the baseline;
none of the kernels' time depends on the values."""
import argparse
import pathlib
import sys

REPO = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

import torch                                     # noqa: E402

import benchlib                                  # noqa: E402
import nb_asr_amd as nb                          # noqa: E402
from nb_asr_amd import hip, ops, optim           # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=50)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    benchlib.need_device('bench_optim.py')
    torch.manual_seed(0)
    model = nb.get_model(benchlib.ARCH, use_rnn=True, dropout_rate=0.0, gpu=0)
    params = list(model.parameters())
    flagged = [i for i, p in enumerate(params) if any(p is m.conv.weight for m in model.modules() if isinstance(m, ops.PadConvRelu))]
    grads = [1e-2 * torch.randn_like(p) for p in params]
    for p, g in zip(params, grads):
        p.grad = g.clone()
    twin = [p.detach().clone().requires_grad_() for p in params]
    for q, g in zip(twin, grads):
        q.grad = g.clone()
    ours = optim.reference_optimizer(model, lr=1e-4)
    theirs = torch.optim.Adam(twin, lr=1e-4, eps=1e-7)

    def hip_steps():
        for _ in range(args.calls):
            ours.step()

    def torch_steps():
        for _ in range(args.calls):
            reg = 0.01 * sum(torch.norm(twin[i]) for i in flagged)
            reg.backward()
            torch.nn.utils.clip_grad_norm_(twin, 5)
            theirs.step()

    # warm-up: code objects, allocator, optimiser state
    (a, a_lo, a_hi), (b, b_lo, b_hi) = (benchlib.summary(t) for t in benchlib.alternate([hip_steps, torch_steps], reps=args.reps, warmup=1))
    n_bytes = 4 * sum(p.numel() for p in params)
    per = lambda ms: round(ms / args.calls, 4)
    row = {'tensors': len(params), 'weight_norm_tensors': len(flagged), 'parameter_MB': round(n_bytes / 1e6, 1), 'calls_per_window': args.calls,
           'windows': args.reps, 'build_id': hip.build_id(),
           'hip_step_ms': per(a), 'hip_step_ms_range': [per(a_lo), per(a_hi)],
           'torch_recipe_ms': per(b), 'torch_recipe_ms_range': [per(b_lo), per(b_hi)],
           'hip_over_torch': round(a / b, 3), 'bytes_per_step': 9 * n_bytes,
           'hip_TB_per_s': round(9 * n_bytes / (a / args.calls * 1e-3) / 1e12, 3),
           'torch_TB_per_s': round(9 * n_bytes / (b / args.calls * 1e-3) / 1e12, 3)}
    benchlib.write_out(args.out, [benchlib.emit([], row)])


if __name__ == '__main__':
    main()
