#!/usr/bin/env python3
"""Time of one training step (training-mode forward + CTC loss + loss.backward() + optimiser step) on the differentiable path.

    python tools/ubench/train_step.py [--batch 16 --frames 400] [--optimizer sgd|adam-torch|adam-hip]

--optimizer sgd (the default, as before): torch.optim.SGD, no regulariser, no clipping.  The two Adam choices run the reference's full
recipe (trainer.py:221-225): adam-torch adds 0.01 * sum(torch.norm(conv.weight)) to the loss, clips with clip_grad_norm_(params, 5) and
steps torch.optim.Adam(lr=1e-4, eps=1e-7); adam-hip does all three in optim.reference_optimizer(model).step().
"""
import argparse
import json
import pathlib
import sys
import time

import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parents[2]))
import nb_asr_amd as nb  # noqa: E402
from nb_asr_amd import ctc, ops, optim  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--batch', type=int, default=16)
ap.add_argument('--frames', type=int, default=400)
ap.add_argument('--steps', type=int, default=3)
ap.add_argument('--optimizer', choices=('sgd', 'adam-torch', 'adam-hip'), default='sgd')
args = ap.parse_args()
torch.manual_seed(0)
model = nb.get_model([[1, 0], [1, 0, 0], [1, 0, 0, 0]], use_rnn=True, dropout_rate=0.0, gpu=0).train()
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
times = []
for step in range(args.steps + 1):
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
    times.append(time.perf_counter() - t0)
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
print(json.dumps({'optimizer': args.optimizer, 'batch': args.batch, 'frames': args.frames, 'train_step_ms': round(1e3 * min(times[1:]), 1), 'first_step_ms': round(1e3 * times[0], 1),
                  'inference_forward_ms': round(1e3 * infer, 2), 'loss': float(loss), 'peak_memory_GB': round(torch.cuda.max_memory_allocated() / 1e9, 2)}))
