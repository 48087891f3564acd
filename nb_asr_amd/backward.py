"""The host side of csrc/backward.hip: the two backward passes that are algorithms rather than one entry point, the
dense k = 8 / per-frame linear maps and the LSTM's BPTT.  They build column matrices, choose between the fp16-split and the exact-fp32
GEMM route (``hip.dense_mode()``) and issue half a dozen launches each, all through wrappers of ``nb_asr_amd.hip``; the backward passes
that ARE one entry point (grouped conv, LayerNorm) are wrappers there.  ``autograd.py`` calls both."""
import torch

from . import hip


def split_gemm_t(x3, cols, w):
    """(w (rows, K) . x3 (batch, K, ld))^T on the fp16 matrix cores, fp32-accurate two-term split -> (cols, batch, rows).
    This is the GEMM of the LSTM input projection (``hip.lstm_input_projection_packed``) with a zero bias: ``w`` stands in for w_ih
    and is packed per call, ``x3`` is pre-split per column tile, ``cols`` <= ld of its columns are frames, and the product is stored
    time-major, i.e. transposed.  That entry point takes 4 * hidden rows with hidden % 4 == 0: ``w`` gets zero rows up to a multiple
    of 16 (only where rows % 16 != 0), ``hidden`` = padded rows // 4, and the padding is sliced off the result."""
    rows, k = w.shape
    batch, _, ld = x3.shape
    r_pad = (rows + 15) & ~15
    if r_pad != rows:
        w = torch.cat([w, w.new_zeros(r_pad - rows, k)])
    zero = torch.zeros(r_pad, device=x3.device, dtype=torch.float32)
    out_t = torch.empty(max(ld, 1), batch, r_pad, device=x3.device, dtype=torch.float32)
    hip.lstm_input_projection_packed(x3, cols, hip.pack_pointwise_weights(w.contiguous()), zero, zero, out_t, r_pad // 4,
                                     hip.pointwise_workspace(batch, k, ld, x3.device))
    return out_t[:max(cols, 1), :, :rows]


def _gemm_f32(x3, cols, w, y):
    """y (1, c_out, ld_out) = w (c_out, c_in) . x3 (1, c_in, ld_in), ``cols`` columns of it: the exact-fp32 MFMA GEMM."""
    return hip.pointwise_linear(x3, cols, w, torch.zeros(w.shape[0], device=w.device, dtype=torch.float32), y)


def dense_conv1d_backward(x, weight, y, dy, frames_in, stride, need_dx=True, need_dw=True, activation=True):
    """Backward of ``y = min(relu(conv1d(zero_pad(x), weight, bias, stride)), 20)`` for the dense k = 8 downsample convs (stride 1 | 2) and
    the per-frame ``linear`` op (k = 1): x (B, C_in, ld_in), y / dy (B, C_out, ld_out) pitched -> (dx, dw, db).  ``activation=False``: the map
    without ReLU / clamp (the CTC head).

    Correctness-first.  Weight and bias gradients: ONE (C_out, B * T') x (B * T', C_in * k + 1) GEMM on a materialised
    column matrix.  Input gradient of the k = 8 convs: ONE (C_in * 8, C_out) x (C_out, B * T') GEMM, then a fold of the 8 tap rows onto
    the input frames (nbasr_conv_fold).  Both GEMMs run on the fp16 matrix cores with the fp32-accurate two-term split;
    ``NBASR_DENSE_MODE=f32`` keeps every product on the exact-fp32 MFMA GEMMs of the forward (there the input gradient is a stride-1 conv
    of the zero-stuffed, masked output gradient with the flipped, channel-transposed kernel)."""
    b, c_in, ld_in = x.shape
    c_out, _, kernel = weight.shape if weight.dim() == 3 else (weight.shape[0], weight.shape[1], 1)
    frames_out = (frames_in + stride - 1) // stride
    lpad = hip.pad_amounts(kernel, 1, stride)[0]
    split = hip.dense_mode() != 'f32'
    dz = hip.relu_clamp_backward(y, dy, torch.empty_like(y)) if activation else dy       # a plain linear map (the CTC head): no mask
    dx = dw = db = None
    if need_dx:
        dx = torch.empty(b, c_in, ld_in, device=x.device, dtype=torch.float32)
        zero = torch.zeros(c_in, device=x.device, dtype=torch.float32)
        if kernel == 1:
            hip.pointwise_linear(dz, frames_in, weight.detach().reshape(c_out, c_in).t().contiguous(), zero, dx)
        elif kernel == 8 and (c_in * kernel) % 16 == 0 and split:
            # ONE split GEMM: rows (ci, tap) of w^T times the masked output gradient, stored time-major, every tap's contribution to dx in its own row;
            # nbasr_conv_fold adds the 8 (stride 1) or 4 (stride 2) rows that land on one input frame.  No zero-stuffing: half the products at stride 2
            wt = weight.detach().permute(1, 2, 0).reshape(c_in * kernel, c_out)
            hip.conv_fold(split_gemm_t(dz, frames_out, wt), dx, frames_in, frames_out, kernel, stride, lpad)
        else:
            up = torch.empty(b, c_out, ld_in, device=x.device, dtype=torch.float32)
            hip.zero_stuff(dz, up, frames_out, frames_in, stride, 0)
            wf = weight.detach().flip(2).permute(1, 0, 2).contiguous()                 # (C_in, C_out, k): flipped taps, channels swapped
            hip.dense_conv1d_linear(up, frames_in, wf, zero, dx, kernel - 1 - lpad)
    if need_dw:
        t_pad = hip.round_up4(max(frames_out, 1))
        ld_cols = hip.round_up4(c_in * kernel + 1)
        cols = torch.empty(1, b * t_pad, ld_cols, device=x.device, dtype=torch.float32)
        hip.conv_cols(x, cols, frames_in, frames_out, t_pad, kernel, stride, lpad)
        rows = torch.empty(c_out, b * t_pad, device=x.device, dtype=torch.float32)
        hip.rows_of_channels(dz, rows, frames_out, t_pad)
        if split:
            # the (C_out, B T') x (B T', C_in k + 1) product as a split GEMM ("weights" = the masked output gradient, "x" = the column
            # matrix), delivered transposed: (C_in k + 1, C_out).  3-5 x the exact-fp32 MFMA GEMM, which was half of a training step
            out = split_gemm_t(cols, c_in * kernel + 1, rows)[:, 0].t()
        else:
            out = _gemm_f32(cols, c_in * kernel + 1, rows, torch.empty(1, c_out, ld_cols, device=x.device, dtype=torch.float32))[0]
        dw = out[:, : c_in * kernel].reshape(weight.shape).contiguous()
        db = out[:, c_in * kernel].contiguous()
    return dx, dw, db


def lstm_backward(xp, frames, gates, h_out, w_ih, w_hh, dh_out):
    """BPTT of the single-layer LSTM (reference model.py:100,118-121): xp (B, C, ld) the layer input, gates (T, B, 4H) its saved input
    projection (both biases included), h_out (B, T, H) the saved output, dh_out (B, T, H) -> (dx (B, C, T), dw_ih, dw_hh, db).

    Correctness first: gate pre-activations of all frames are recomputed from the saved h by ONE GEMM, a serial
    scan restores the cell states, the reverse recurrence is T launches of a step kernel that forms w_hh^T . dpre of the next frame in place, and the weight / input gradients
    are batched GEMMs -- on the fp16 matrix cores with the fp32-accurate two-term split (``NBASR_DENSE_MODE=f32``: the exact-fp32 MFMA GEMM
    nbasr_pointwise_linear); tensor re-layouts are torch copies."""
    b, c, _ = xp.shape
    t_n, hidden = frames, w_hh.shape[1]
    g4 = 4 * hidden
    dev, f32 = xp.device, torch.float32
    if hidden % 4:
        raise hip.HipError('lstm_backward: hidden must be a multiple of 4')
    ldb = hip.round_up4(b)
    n = t_n * ldb                                              # GEMM column count; (frame, utterance) pairs, utterance innermost
    split = hip.dense_mode() != 'f32'
    # h_(t-1) for every (t, b): rows of the (T * ldb, H) matrix, zero for t = 0 and for the pitch utterances
    hp = torch.zeros(t_n, ldb, hidden, device=dev, dtype=f32)
    if t_n > 1:
        hp[1:, :b] = h_out[:, : t_n - 1].permute(1, 0, 2)
    hp_t = hp.reshape(n, hidden).t().contiguous().view(1, hidden, n)
    if split:
        pre = split_gemm_t(hp_t, n, w_hh.detach())[:, 0].t().contiguous().view(g4, t_n, ldb)
    else:
        pre = _gemm_f32(hp_t, n, w_hh.detach().contiguous(), torch.empty(1, g4, n, device=dev, dtype=f32)).view(g4, t_n, ldb)
    pre[:, :, :b] += gates[:t_n].permute(2, 0, 1)             # + input projection and biases
    cells = torch.zeros(hidden, t_n, ldb, device=dev, dtype=f32)
    hip.lstm_gate_scan(pre, cells, b)                          # pre is overwritten in place by the gate activations
    dho = torch.zeros(hidden, t_n, ldb, device=dev, dtype=f32)
    dho[:, :, :b] = dh_out.detach().permute(2, 1, 0)
    dpre = torch.empty(g4, t_n, ldb, device=dev, dtype=f32)
    dc = torch.zeros(hidden, ldb, device=dev, dtype=f32)
    hip.lstm_backward_step(dho, w_hh.detach().t().contiguous(), dc, pre, cells, dpre, b, -1)    # t = -1: frames T-1 .. 0 in one call
    d2 = dpre.view(g4, n)
    ldc = hip.round_up4(c + 1)
    xh = torch.zeros(t_n, ldb, ldc + hidden if split else ldc, device=dev, dtype=f32)        # (x | 1), on the split route (x | 1 | h_prev)
    xh[:, :b, :c] = xp[:, :, :t_n].permute(2, 0, 1)
    xh[:, :b, c] = 1.0
    if split:
        # (dw_ih | db | dw_hh) (4H, C + 1 + H) = dpre (4H, n) . (x | 1 | h_prev) (n, .): ONE GEMM, dpre packed once
        xh[:, :, ldc:] = hp
        wb = split_gemm_t(xh.view(1, n, ldc + hidden), ldc + hidden, d2)[:, 0].t()
        dw_hh = wb[:, ldc:].contiguous()
        # dx (C, n) = w_ih^T (C, 4H) . dpre (4H, n), delivered transposed: (n, C)
        dx = split_gemm_t(dpre.view(1, g4, n), n, w_ih.detach().t())[:, 0].view(t_n, ldb, c)[:, :b].permute(1, 2, 0).contiguous()
    else:
        # dw_hh (4H, H) = dpre (4H, n) . h_prev (n, H);  (dw_ih | db) (4H, C + 1) = dpre . (x | 1);  dx (C, n) = w_ih^T (C, 4H) . dpre (4H, n)
        dw_hh = _gemm_f32(hp.view(1, n, hidden), hidden, d2, torch.empty(1, g4, hidden, device=dev, dtype=f32))[0]
        wb = _gemm_f32(xh.view(1, n, ldc), c + 1, d2, torch.empty(1, g4, ldc, device=dev, dtype=f32))[0]
        dxc = _gemm_f32(dpre.view(1, g4, n), n, w_ih.detach().t().contiguous(), torch.empty(1, c, n, device=dev, dtype=f32))[0]
        dx = dxc.view(c, t_n, ldb)[:, :, :b].permute(2, 0, 1).contiguous()
    return dx, wb[:, :c].contiguous(), dw_hh, wb[:, c].contiguous()
