"""The single-launch backward building blocks; backward.py strings the last eight together (nbasr.h says what each
computes).  The optimisation step's signatures are registered here too; its wrappers, with their tables, are optim.py.  ``dropout`` is the
counter-based dropout launch of the training path; its seed and call counter are kept by nb_asr_amd/dropout.py."""
import ctypes

import torch

from . import SIGNATURES, HipError, load_library, _call, _scratch, _stream, _dev, _opt, _skips3, _signed64, _c_float_p, _c_int, _c_stream

SIGNATURES.update({
    'nbasr_grouped_conv1d_backward_workspace_bytes': (ctypes.c_size_t, [_c_int] * 4),
    'nbasr_grouped_conv1d_backward': (_c_int, [_c_float_p] * 8 + [_c_int] * 7 + [_c_stream]),
    'nbasr_layernorm_backward_workspace_bytes': (ctypes.c_size_t, [_c_int] * 3),
    'nbasr_layernorm_channels_backward': (_c_int, [_c_float_p] * 8 + [_c_int] * 4 + [_c_stream]),
    'nbasr_relu_clamp_backward': (_c_int, [_c_float_p] * 3 + [ctypes.c_longlong, _c_stream]),
    'nbasr_zero_stuff': (_c_int, [_c_float_p] * 2 + [_c_int] * 7 + [_c_stream]),
    'nbasr_conv_fold': (_c_int, [_c_float_p] * 2 + [_c_int] * 8 + [_c_stream]),
    'nbasr_dense_conv1d_linear': (_c_int, [_c_float_p] * 4 + [_c_int] * 8 + [_c_stream]),
    'nbasr_conv_cols': (_c_int, [_c_float_p] * 2 + [_c_int] * 10 + [_c_stream]),
    'nbasr_rows_of_channels': (_c_int, [_c_float_p] * 2 + [_c_int] * 5 + [_c_stream]),
    'nbasr_lstm_gate_scan': (_c_int, [_c_float_p] * 2 + [_c_int] * 4 + [_c_stream]),
    'nbasr_lstm_backward_step': (_c_int, [_c_float_p] * 6 + [_c_int] * 5 + [_c_stream]),
    'nbasr_optim_table_bytes': (ctypes.c_size_t, [_c_int] * 2),
    'nbasr_optim_workspace_bytes': (ctypes.c_size_t, [_c_int] * 2),
    'nbasr_optim_adam_step': (_c_int, [ctypes.c_void_p, _c_int, _c_int, ctypes.c_void_p, _c_float_p] + [ctypes.c_double] * 5 + [_c_stream]),
    'nbasr_dropout': (_c_int, [_c_float_p] * 5 + [_c_int] * 3 + [ctypes.c_double] + [ctypes.c_longlong] * 3 + [_c_stream]),
})


def dropout(x, y, frames, p, seed, call, skips=(), row0=0):
    """y[..., :frames] = x * (kept ? 1 / (1 - p) : 0) (+ up to three skips, the node's sum left to right) with the counter-based mask of
    (seed, call, row0 + row, frame): nbasr.h "dropout".  x, y and the skips: float32 tensors of one shape (..., ld), rows = the product
    of the leading dimensions; y may be x.  The pitch columns of y are not written.  Backward is the same call on the gradient."""
    ld = x.shape[-1]
    if tuple(y.shape) != tuple(x.shape) or any(tuple(s.shape) != tuple(x.shape) for s in skips):
        raise HipError(f'dropout: y and the skips must have the shape of x, {tuple(x.shape)}')
    if len(skips) > 3:
        raise HipError(f'dropout: at most three skips per launch (got {len(skips)})')
    s = _skips3(skips)
    _call('nbasr_dropout', _dev(x, 'x'), _opt(s[0], 'skip0'), _opt(s[1], 'skip1'), _opt(s[2], 'skip2'), _dev(y, 'y'), x.numel() // max(ld, 1),
          frames, ld, float(p), _signed64(seed), _signed64(call), int(row0), _stream(x))
    return y


def grouped_conv1d_backward(x, weight, z, dz, frames, groups, kernel, dilation, need_dx=True, need_dw=True):
    """Gradients of z = min(relu(grouped_conv(x, weight) + bias), 20) given dz: (dx or None, dw or None, db or None).
    x, z, dz: (B, C, ld) float32 pitched tensors (z = the op's output; dz's pitch columns zero)."""
    b, c, ld = z.shape
    dx = torch.empty_like(z) if need_dx else None
    dw = torch.empty_like(weight) if need_dw else None
    db = torch.empty(c, dtype=torch.float32, device=z.device) if need_dw else None
    ws_bytes = load_library().nbasr_grouped_conv1d_backward_workspace_bytes
    ws = _scratch(ws_bytes(max(b, 1), c, groups, kernel), z.device, torch.float32, 16) if need_dw else None
    _call('nbasr_grouped_conv1d_backward', _opt(x, 'x'), _dev(weight, 'weight'), _dev(z, 'z'), _dev(dz, 'dz'), _opt(dx, 'dx'), _opt(dw, 'dw'),
          _opt(db, 'db'), _opt(ws, 'workspace'), b, c, frames, ld, groups, kernel, dilation, _stream(z))
    return dx, dw, db


def layernorm_channels_backward(x, stats, gamma, dy, frames):
    """(dx, dgamma, dbeta) of y = LayerNorm_channels(x) given dy; stats = channel_stats(x)."""
    b, c, ld = x.shape
    dx = torch.empty_like(x)
    dgamma = torch.empty(c, dtype=torch.float32, device=x.device)
    dbeta = torch.empty(c, dtype=torch.float32, device=x.device)
    ws = _scratch(load_library().nbasr_layernorm_backward_workspace_bytes(max(b, 1), c, max(ld, 4)), x.device, torch.float32, 16)
    _call('nbasr_layernorm_channels_backward', _dev(x, 'x'), _dev(stats, 'stats'), _dev(gamma, 'gamma'), _dev(dy, 'dy'), _dev(dx, 'dx'),
          _dev(dgamma, 'dgamma'), _dev(dbeta, 'dbeta'), _dev(ws, 'workspace'), b, c, frames, ld, _stream(x))
    return dx, dgamma, dbeta


def relu_clamp_backward(y, dy, dz):
    _call('nbasr_relu_clamp_backward', _dev(y, 'y'), _dev(dy, 'dy'), _dev(dz, 'dz'), y.numel(), _stream(y))
    return dz


def zero_stuff(dz, up, frames, frames_up, stride, shift):
    b, c, ld = dz.shape
    _call('nbasr_zero_stuff', _dev(dz, 'dz'), _dev(up, 'up'), b * c, frames, ld, frames_up, up.shape[2], stride, shift, _stream(dz))


def dense_conv1d_linear(x, frames, weight, bias, y, lpad):
    b, c_in, ld_in = x.shape
    c_out, _, kernel = weight.shape
    _call('nbasr_dense_conv1d_linear', _dev(x, 'x'), _dev(weight, 'weight'), _dev(bias, 'bias'), _dev(y, 'y'), b, c_in, frames, ld_in, c_out,
          y.shape[2], kernel, lpad, _stream(x))


def conv_cols(x, cols, frames_in, frames_out, t_pad, taps, stride, lpad):
    b, c_in, ld_in = x.shape
    _call('nbasr_conv_cols', _dev(x, 'x'), _dev(cols, 'cols'), b, c_in, frames_in, ld_in, frames_out, t_pad, taps, stride, lpad, cols.shape[-1], _stream(x))


def rows_of_channels(dz, rows, frames, t_pad):
    b, c, ld = dz.shape
    _call('nbasr_rows_of_channels', _dev(dz, 'dz'), _dev(rows, 'rows'), b, c, frames, ld, t_pad, _stream(dz))


def conv_fold(cols, dx, frames_in, frames_out, taps, stride, lpad):
    b, c_in, ld_in = dx.shape
    _call('nbasr_conv_fold', _dev(cols, 'cols'), _dev(dx, 'dx'), b, c_in, frames_in, ld_in, frames_out, taps, stride, lpad, _stream(dx))


def lstm_gate_scan(pre, cells, batch):
    """Overwrites pre (4H, T, ldb) with the gate activations; cells (H, T, ldb) <- c_t."""
    hidden, frames, ldb = cells.shape
    _call('nbasr_lstm_gate_scan', _dev(pre, 'pre'), _dev(cells, 'cells'), hidden, frames, batch, ldb, _stream(pre))


def lstm_backward_step(dh_out, w_hh_t, dc, acts, cells, dpre, batch, t):
    hidden, frames, ldb = cells.shape
    _call('nbasr_lstm_backward_step', _dev(dh_out, 'dho'), _dev(w_hh_t, 'w_hh_t'), _dev(dc, 'dc'), _dev(acts, 'acts'), _dev(cells, 'cells'),
          _dev(dpre, 'dpre'), hidden, frames, batch, ldb, t, _stream(dh_out))
