#!/usr/bin/env python3
"""Time of one training step (training-mode forward + CTC loss + loss.backward() + optimiser step) on the differentiable path.

    python tools/ubench/train_step.py [--batch 16 --frames 400] [--optimizer sgd|adam-torch|adam-hip]
                                      [--dropout 0.2 --dropout-backend aten|hip|aten,hip] [--out profiles/dropout/train_step.json]

--optimizer sgd (the default, as before): torch.optim.SGD, no regulariser, no clipping.  The two Adam choices run the reference's full
recipe (trainer.py:221-225): adam-torch adds 0.01 * sum(torch.norm(conv.weight)) to the loss, clips with clip_grad_norm_(params, 5) and
steps torch.optim.Adam(lr=1e-4, eps=1e-7); adam-hip does all three in optim.reference_optimizer(model).step().

--dropout P builds the model with that rate (the reference trains with 0.2); --dropout-backend picks who drops (nb_asr_amd.dropout.use).
With both backends, comma-separated, they take turns step by step in this one process, and the median, smallest and largest step time
of each are reported side by side.
"""
import argparse
import json
import pathlib
import statistics
import sys
import time

import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parents[2]))
import nb_asr_amd as nb  # noqa: E402
from nb_asr_amd import ctc, dropout, ops, optim  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--batch', type=int, default=16)
ap.add_argument('--frames', type=int, default=400)
ap.add_argument('--steps', type=int, default=3)
ap.add_argument('--optimizer', choices=('sgd', 'adam-torch', 'adam-hip'), default='sgd')
ap.add_argument('--dropout', type=float, default=0.0)
ap.add_argument('--dropout-backend', default='aten', help="aten, hip, or both as 'aten,hip': they alternate step by step")
ap.add_argument('--out', default=None)
args = ap.parse_args()
backends = args.dropout_backend.split(',')
torch.manual_seed(0)
dropout.manual_seed(0)
model = nb.get_model([[1, 0], [1, 0, 0], [1, 0, 0, 0]], use_rnn=True, dropout_rate=args.dropout, gpu=0).train()
x = torch.randn(args.batch, 80, args.frames, device='cuda:0')
t_out = (args.frames + 3) // 4
targets = torch.randint(1, 49, (args.batch, 20), dtype=torch.int32, device='cuda:0')
tl = torch.full((args.batch,), 20, dtype=torch.int32, device='cuda:0')
ol = torch.full((args.batch,), t_out, dtype=torch.int32, device='cuda:0')
if args.optimizer == 'sgd':
    opt = torch.optim.SGD(model.parameters(), lr=1e-3)
elif args.optimizer == 'adam-torch':
    opt = torch.optim.Adam(model.parameters(), lr=1e-4, eps=1e-7)
    convs = [m.conv.weight for m in model.modules() if isinstance(m, ops.PadConvRelu)]
else:
    opt = optim.reference_optimizer(model, lr=1e-4)
times = {b: [] for b in backends}
for step in range(args.steps + 1):
    for b in backends:
        with dropout.use(b):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            loss = ctc.training_loss(model(x), ol, targets, tl)
            opt.zero_grad()
            if args.optimizer == 'adam-torch':
                (loss + 0.01 * sum(torch.norm(w) for w in convs)).backward()
                torch.nn.utils.clip_grad_norm_(model.parameters(), 5)
            else:
                loss.backward()
            opt.step()
            torch.cuda.synchronize()
            times[b].append(time.perf_counter() - t0)
with torch.no_grad():
    model.eval()
    for _ in range(3):
        model(x)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(5):
        model(x)
    torch.cuda.synchronize()
    infer = (time.perf_counter() - t0) / 5
row = {'optimizer': args.optimizer, 'batch': args.batch, 'frames': args.frames, 'dropout': args.dropout, 'dropout_backend': args.dropout_backend,
       'train_step_ms': round(1e3 * min(times[backends[0]][1:]), 1), 'first_step_ms': round(1e3 * times[backends[0]][0], 1),
       'inference_forward_ms': round(1e3 * infer, 2), 'loss': float(loss), 'peak_memory_GB': round(torch.cuda.max_memory_allocated() / 1e9, 2)}
if len(backends) > 1:
    row['steps_per_backend'] = args.steps
    for b in backends:              # the first step of each (code objects, allocator) is left out
        row[f'train_step_ms_{b}'] = {'median': round(1e3 * statistics.median(times[b][1:]), 1), 'min': round(1e3 * min(times[b][1:]), 1),
                                     'max': round(1e3 * max(times[b][1:]), 1)}
print(json.dumps(row))
if args.out:
    pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    pathlib.Path(args.out).write_text(json.dumps(row, indent=1) + '\n')
