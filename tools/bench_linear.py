#!/usr/bin/env python3
"""The per-frame GEMM (gemm_pointwise.hip) at the model's shapes, image pass + GEMM per call, for both operand schemes:
the `linear` node op at the four block shapes (fp32 rows: beside the exact-fp32 MFMA GEMM) and the LSTM input projection."""
import pathlib, statistics, sys
import torch
sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))
import benchlib
from nb_asr_amd import hip
DEV = 'cuda:0'
BF16 = torch.bfloat16
B = 64


def timeit(fn):
    return statistics.median(benchlib.alternate([fn], reps=10, warmup=3)[0])


def report(what, c, t, gf, times):
    print(f'{what} C={c:5d} T={t:5d}: ' + '   '.join(f'{name} {ms * 1e3:7.1f} us ({gf / ms:6.1f} TF)' for name, ms in times), flush=True)


for c, t in ((600, 1000), (800, 1000), (1000, 500), (1200, 250)):
    gf = 2.0 * B * t * c * c / 1e9
    x = torch.randn(B, c, hip.round_up4(t), device=DEV)
    w, bias = torch.randn(c, c, device=DEV) * 0.03, torch.randn(c, device=DEV)
    y = torch.empty_like(x)
    packed, ws = hip.pack_pointwise_weights(w), hip.pointwise_workspace(B, c, x.shape[2], DEV)
    w3 = w.unsqueeze(-1).contiguous()
    t16 = timeit(lambda: hip.linear_fused_packed(x, t, packed, c, bias, (), y, ws))
    t32 = timeit(lambda: hip.dense_conv1d_fused(x, t, w3, bias, (), y, 1))
    report('linear', c, t, gf, (('f16x2', t16), ('fp32', t32)))
    xb = torch.randn(B, c, hip.row_pitch(t, BF16), device=DEV).to(BF16)
    yb = torch.empty_like(xb)
    packed, ws = hip.pack_pointwise_weights_bf16(w.to(BF16).float()), hip.pointwise_bf16_workspace(B, c, xb.shape[2], DEV)
    report('linear', c, t, gf, (('bf16', timeit(lambda: hip.linear_fused_bf16(xb, t, packed, c, bias, (), yb, ws))),))

c, t, hidden = 1200, 250, 500
gf = 2.0 * B * t * c * 4 * hidden / 1e9
w, b_ih, b_hh = torch.randn(4 * hidden, c, device=DEV) * 0.03, torch.randn(4 * hidden, device=DEV), torch.randn(4 * hidden, device=DEV)
gates = torch.empty(t, B, 4 * hidden, device=DEV)
x = torch.randn(B, c, hip.round_up4(t), device=DEV)
packed, ws = hip.pack_pointwise_weights(w), hip.pointwise_workspace(B, c, x.shape[2], DEV)
report('lstm projection', c, t, gf, (('f16x2', timeit(lambda: hip.lstm_input_projection_packed(x, t, packed, b_ih, b_hh, gates, hidden, ws))),))
xb = torch.randn(B, c, hip.row_pitch(t, BF16), device=DEV).to(BF16)
packed, ws = hip.pack_pointwise_weights_bf16(w.to(BF16).float()), hip.pointwise_bf16_workspace(B, c, xb.shape[2], DEV)
report('lstm projection', c, t, gf, (('bf16', timeit(lambda: hip.lstm_input_projection_bf16(xb, t, packed, b_ih, b_hh, gates, hidden, ws))),))
