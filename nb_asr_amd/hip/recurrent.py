"""The per-frame linear maps on the matrix cores (both operand schemes), the LSTM input projection, every form of the recurrence, the head."""
import collections
import ctypes
import functools

import torch

from . import (SIGNATURES, HipError, load_library, _call, _scratch, _opaque, _stream, _dev, _opt, _act, _act_opt, _ln, _skips3,
               _c_float_p, _c_int, _c_stream, _c_ln_p)

SIGNATURES.update({
    # per-frame linear maps: the 2 x fp16 split of fp32 rows ...
    'nbasr_pointwise_packed_weights_bytes': (ctypes.c_size_t, [_c_int] * 2),
    'nbasr_pointwise_workspace_bytes': (ctypes.c_size_t, [_c_int] * 3),
    'nbasr_pack_pointwise_weights': (_c_int, [_c_float_p] * 2 + [_c_int] * 2 + [_c_stream]),
    'nbasr_linear_fused_packed': (_c_int, [_c_float_p] * 8 + [_c_int] * 5 + [_c_ln_p, _c_int, _c_int, _c_stream]),
    'nbasr_lstm_input_projection_packed': (_c_int, [_c_float_p] * 6 + [_c_int] * 5 + [_c_ln_p, _c_stream]),
    'nbasr_lstm_input_projection_packed_into': (_c_int, [_c_float_p] * 6 + [_c_int] * 5 + [_c_ln_p, _c_int, _c_int, _c_stream]),
    # ... and bf16 rows, one term
    'nbasr_pointwise_bf16_weights_bytes': (ctypes.c_size_t, [_c_int] * 2),
    'nbasr_pointwise_bf16_workspace_bytes': (ctypes.c_size_t, [_c_int] * 3),
    'nbasr_pack_pointwise_weights_bf16': (_c_int, [_c_float_p] * 2 + [_c_int] * 2 + [_c_stream]),
    'nbasr_linear_fused_bf16': (_c_int, [_c_float_p] * 8 + [_c_int] * 5 + [_c_ln_p, _c_int, _c_int, _c_stream]),
    'nbasr_lstm_input_projection_bf16': (_c_int, [_c_float_p] * 6 + [_c_int] * 5 + [_c_ln_p, _c_stream]),
    # LSTM + head
    'nbasr_lstm_input_projection': (_c_int, [_c_float_p] * 5 + [_c_int] * 5 + [_c_ln_p, _c_stream]),
    'nbasr_lstm_packed_whh_bytes': (ctypes.c_size_t, [_c_int]),
    'nbasr_lstm_pack_whh': (_c_int, [_c_float_p] * 2 + [_c_int, _c_stream]),
    'nbasr_lstm_recurrence_packed': (_c_int, [_c_float_p] * 4 + [_c_int] * 3 + [_c_stream]),
    'nbasr_lstm_seq_workspace_bytes': (ctypes.c_size_t, [_c_int] * 2),
    'nbasr_lstm_recurrence_seq': (_c_int, [_c_float_p] * 5 + [_c_int] * 4 + [_c_stream]),
    'nbasr_lstm_seq_status': (_c_int, [_c_float_p, _c_stream]),
    'nbasr_lstm_packed_whh16_bytes': (ctypes.c_size_t, [_c_int]),
    'nbasr_lstm_pack_whh16': (_c_int, [_c_float_p] * 2 + [_c_int, _c_stream]),
    'nbasr_lstm_xcd_workspace_bytes': (ctypes.c_size_t, [_c_int] * 2),
    'nbasr_lstm_recurrence_xcd': (_c_int, [_c_float_p] * 5 + [_c_int] * 4 + [_c_stream]),
    'nbasr_lstm_recurrence_frames16': (_c_int, [_c_float_p] * 5 + [_c_int] * 3 + [_c_stream]),
    'nbasr_lstm_recurrence_frames16_state': (_c_int, [_c_float_p] * 6 + [_c_int] * 4 + [_c_stream]),
    'nbasr_linear_head': (_c_int, [_c_float_p] * 4 + [_c_int] * 3 + [_c_stream]),
    'nbasr_linear_head_bct': (_c_int, [_c_float_p] * 4 + [_c_int] * 5 + [_c_ln_p, _c_stream]),
})


def lstm_forward(x, frames, w_ih, w_hh, b_ih, b_hh, gates_ws, cell_ws, h_out, ln=None):
    """nn.LSTM forward as its two library calls on one stream: the exact-fp32 input projection, then the per-frame recurrence."""
    lstm_input_projection(x, frames, w_ih, b_ih, b_hh, gates_ws, w_hh.shape[1], ln)
    return lstm_recurrence(gates_ws, w_hh, cell_ws, h_out)


def lstm_input_projection(x, frames, w_ih, b_ih, b_hh, gates_ws, hidden, ln=None):
    """gates_ws (frames, batch, 4*hidden) <- x . w_ih^T + b_ih + b_hh for all frames (first half of lstm_forward)."""
    b, c_in, ld = x.shape
    _call('nbasr_lstm_input_projection', _dev(x, 'x'), _dev(w_ih, 'w_ih'), _dev(b_ih, 'b_ih'), _dev(b_hh, 'b_hh'), _dev(gates_ws, 'gates_ws'),
          b, c_in, frames, ld, hidden, _ln(ln), _stream(x))
    return gates_ws


def lstm_pack_whh(w_hh):
    """(4H, H) recurrent weight -> opaque uint8 tensor in the operand-fragment order of the step kernel."""
    hidden = w_hh.shape[1]
    packed = torch.empty(load_library().nbasr_lstm_packed_whh_bytes(hidden), dtype=torch.uint8, device=w_hh.device)
    _call('nbasr_lstm_pack_whh', _dev(w_hh, 'w_hh'), packed.data_ptr(), hidden, _stream(w_hh))
    return packed


def _check_whh(packed_whh, h_out):
    _opaque(packed_whh, load_library().nbasr_lstm_packed_whh_bytes(h_out.shape[2]),
            'packed_whh must be the uint8 device tensor returned by lstm_pack_whh for this hidden size', exact=True)
    return h_out.shape


def lstm_recurrence_packed(gates_ws, packed_whh, cell_ws, h_out):
    b, frames, hidden = _check_whh(packed_whh, h_out)
    _call('nbasr_lstm_recurrence_packed', _dev(gates_ws, 'gates_ws'), packed_whh.data_ptr(), _dev(cell_ws, 'cell_ws'), _dev(h_out, 'h_out'),
          b, frames, hidden, _stream(h_out))
    return h_out


def lstm_recurrence(gates_ws, w_hh, cell_ws, h_out):
    """h_out (batch, frames, hidden) from the projected gates (second half of lstm_forward), on the current stream; packs w_hh per call
    (a caller that keeps the weight packs it once: lstm_pack_whh + lstm_recurrence_packed)."""
    return lstm_recurrence_packed(gates_ws, lstm_pack_whh(w_hh), cell_ws, h_out)


def lstm_seq_workspace(batch, hidden, device):
    """Workspace of the one-launch recurrence (flags + the exchange images of h), or None where that form does not apply."""
    nbytes = lstm_seq_workspace_bytes(int(batch), int(hidden), device)
    return _scratch(nbytes, device) if nbytes else None


HIP_ERROR_COOPERATIVE_LAUNCH_TOO_LARGE = 720       # hipErrorCooperativeLaunchTooLarge: nbasr_lstm_recurrence_seq passes a refused grid's code through
LSTM_SEQ_INJECT_FAULT = 1       # NBASR_LSTM_SEQ_INJECT_FAULT of nbasr_lstm_recurrence_seq (tests)
LSTM_CONTINUE = 2               # NBASR_LSTM_CONTINUE of nbasr_lstm_recurrence_frames16_state


def lstm_recurrence_seq(gates_ws, packed_whh, cell_ws, h_out, seq_ws, flags=0):
    """lstm_recurrence_packed with all frames in ONE (cooperative) launch: w_hh resident in registers, h exchanged in payload-tagged
    granules; same h_out, bit for bit.  The first int32 of ``seq_ws`` is the status word (non-zero: a step timed out, h_out holds NaN)."""
    b, frames, hidden = _check_whh(packed_whh, h_out)
    need = lstm_seq_workspace_bytes(b, hidden, h_out.device)
    wrong = f'lstm_recurrence_seq: batch={b} hidden={hidden} needs a uint8 device workspace of {need} bytes from lstm_seq_workspace ' \
            '(0 = this form does not apply)'
    if need == 0 or seq_ws is None:
        raise HipError(wrong)
    _opaque(seq_ws, need, wrong)
    _call('nbasr_lstm_recurrence_seq', _dev(gates_ws, 'gates_ws'), packed_whh.data_ptr(), _dev(cell_ws, 'cell_ws'), _dev(h_out, 'h_out'),
          seq_ws.data_ptr(), b, frames, hidden, int(flags), _stream(h_out))
    return h_out


def lstm_seq_workspace_bytes(batch, hidden, device):
    """Workspace of the one-launch recurrence on ``device`` (0: that form does not apply there).  The answer depends on how many
    workgroups THAT device holds at once, and the C query asks the current device: it runs with ``device`` current."""
    with torch.cuda.device(device):
        return load_library().nbasr_lstm_seq_workspace_bytes(batch, hidden)


def lstm_seq_status(seq_ws):
    """Synchronises the current stream and raises HipError if a step of the last one-launch recurrence timed out."""
    _call('nbasr_lstm_seq_status', seq_ws.data_ptr(), _stream(seq_ws))


def lstm_pack_whh16(w_hh):
    """w_hh (4*hidden, hidden) fp32 -> the resident operand image of lstm_recurrence_xcd (two fp16 terms per weight; hidden <= 512)."""
    hidden = w_hh.shape[1]
    nbytes = load_library().nbasr_lstm_packed_whh16_bytes(hidden)
    if w_hh.shape[0] != 4 * hidden or nbytes == 0:
        raise HipError(f'lstm_pack_whh16: w_hh must be (4*hidden, hidden) with hidden <= 512, got {tuple(w_hh.shape)}')
    packed = torch.empty(nbytes, dtype=torch.uint8, device=w_hh.device)
    _call('nbasr_lstm_pack_whh16', _dev(w_hh, 'w_hh'), packed.data_ptr(), hidden, _stream(w_hh))
    return packed


def lstm_xcd_workspace_bytes(batch, hidden):
    return load_library().nbasr_lstm_xcd_workspace_bytes(int(batch), int(hidden))


def lstm_xcd_workspace(batch, hidden, device):
    nbytes = lstm_xcd_workspace_bytes(batch, hidden)
    if nbytes == 0:
        raise HipError(f'lstm_recurrence_xcd does not apply to batch={batch}, hidden={hidden} (hidden <= 512, batch <= 4096)')
    return _scratch(nbytes, device)


def _check_whh16(packed_whh16, xcd_ws, h_out, who, hint=''):
    batch, _, hidden = h_out.shape
    _opaque(packed_whh16, load_library().nbasr_lstm_packed_whh16_bytes(hidden),
            'packed_whh16 must be the uint8 device tensor returned by lstm_pack_whh16 for this hidden size', exact=True)
    need = lstm_xcd_workspace_bytes(batch, hidden)
    wrong = f'{who}: batch={batch} hidden={hidden} needs a uint8 device workspace of {need} bytes from lstm_xcd_workspace{hint}'
    if need == 0:
        raise HipError(wrong)
    _opaque(xcd_ws, need, wrong)
    return h_out.shape


def lstm_recurrence_xcd(gates_ws, packed_whh16, cell_ws, h_out, xcd_ws, flags=0):
    """The recurrence as ONE resident launch, a tile of 16 utterances per XCD, on the fp16 matrix cores (nbasr.h, ABI 6): h_out agrees
    with lstm_recurrence_packed to fp32 round-off.  The status word of ``xcd_ws`` is read by ``lstm_seq_status``."""
    b, frames, hidden = _check_whh16(packed_whh16, xcd_ws, h_out, 'lstm_recurrence_xcd', ' (0 = the form does not apply)')
    _call('nbasr_lstm_recurrence_xcd', _dev(gates_ws, 'gates_ws'), packed_whh16.data_ptr(), _dev(cell_ws, 'cell_ws'), _dev(h_out, 'h_out'),
          xcd_ws.data_ptr(), b, frames, hidden, int(flags), _stream(h_out))
    return h_out


def lstm_recurrence_frames16(gates_ws, packed_whh16, cell_ws, h_out, xcd_ws):
    """lstm_recurrence_xcd's arithmetic as one launch per frame (bit-identical h_out): the form of a pipelined tail and of a demoted plan."""
    b, frames, hidden = _check_whh16(packed_whh16, xcd_ws, h_out, 'lstm_recurrence_frames16')
    _call('nbasr_lstm_recurrence_frames16', _dev(gates_ws, 'gates_ws'), packed_whh16.data_ptr(), _dev(cell_ws, 'cell_ws'), _dev(h_out, 'h_out'),
          xcd_ws.data_ptr(), b, frames, hidden, _stream(h_out))
    return h_out


def lstm_recurrence_frames16_state(gates_ws, packed_whh16, cell_ws, h_out, xcd_ws, h0=None, flags=0):
    """lstm_recurrence_frames16 with carried state: ``flags=LSTM_CONTINUE`` starts frame 0 from c = ``cell_ws`` and h = ``h0``
    ((batch, hidden) float32, None = zeros) instead of zeros (nbasr.h).  flags = 0 and h0 = None: bit-identical to lstm_recurrence_frames16."""
    b, frames, hidden = _check_whh16(packed_whh16, xcd_ws, h_out, 'lstm_recurrence_frames16_state')
    if h0 is not None and h0.numel() != b * hidden:
        raise HipError(f'lstm_recurrence_frames16_state: h0 must hold ({b}, {hidden}) floats')
    _call('nbasr_lstm_recurrence_frames16_state', _dev(gates_ws, 'gates_ws'), packed_whh16.data_ptr(), _dev(cell_ws, 'cell_ws'),
          _dev(h_out, 'h_out'), xcd_ws.data_ptr(), _opt(h0, 'h0'), b, frames, hidden, int(flags), _stream(h_out))
    return h_out


# The two operand schemes of the per-frame maps (gemm_pointwise.hip: one template).  ``act`` / ``act_opt``: the pointer checks of its activations;
# ``pack_name`` / ``workspace_name``: its wrappers as its messages quote them; the rest: its entry points.
_PwScheme = collections.namedtuple('_PwScheme', 'weights_bytes workspace_bytes pack linear projection act act_opt pack_name workspace_name')
_PW_SCHEMES = {
    'f16x2': _PwScheme('nbasr_pointwise_packed_weights_bytes', 'nbasr_pointwise_workspace_bytes', 'nbasr_pack_pointwise_weights',
                       'nbasr_linear_fused_packed', 'nbasr_lstm_input_projection_packed', _dev, _opt, 'pack_pointwise_weights', 'pointwise_workspace'),
    'bf16': _PwScheme('nbasr_pointwise_bf16_weights_bytes', 'nbasr_pointwise_bf16_workspace_bytes', 'nbasr_pack_pointwise_weights_bf16',
                      'nbasr_linear_fused_bf16', 'nbasr_lstm_input_projection_bf16', functools.partial(_act, dtype=torch.bfloat16),
                      functools.partial(_act_opt, dtype=torch.bfloat16), 'pack_pointwise_weights_bf16', 'pointwise_bf16_workspace'),
}


def _pw_pack(scheme, weight):
    """(c_out, c_in) fp32 weight of a per-frame linear map -> opaque uint8 tensor: 2 x fp16 split in LDS-image order + row scales; 'bf16':
    the values of a bf16 weight as bf16 in LDS-image order."""
    c_out, c_in = weight.shape
    packed = torch.empty(getattr(load_library(), _PW_SCHEMES[scheme].weights_bytes)(c_out, c_in), dtype=torch.uint8, device=weight.device)
    _call(_PW_SCHEMES[scheme].pack, _dev(weight, 'weight'), packed.data_ptr(), c_out, c_in, _stream(weight))
    return packed


def _pw_workspace(scheme, batch, c_in, ld, device):
    """Scratch for the pre-split activation image of the scheme's `linear` op and input projection."""
    return _scratch(getattr(load_library(), _PW_SCHEMES[scheme].workspace_bytes)(batch, c_in, ld), device, least=16)


def _pw_check(scheme, packed, ws, c_out, c_in, batch, ld):
    lib, s = load_library(), _PW_SCHEMES[scheme]
    _opaque(packed, getattr(lib, s.weights_bytes)(c_out, c_in), ('packed weights are not the {} image of a ({}, {}) weight', s.pack_name, c_out, c_in),
            exact=True)
    _opaque(ws, getattr(lib, s.workspace_bytes)(batch, c_in, ld), ('workspace too small: allocate it with {}(batch, c_in, ld, device)', s.workspace_name))


def _pw_linear(scheme, x, frames, packed, c_out, bias, skips, y, ws, ln=None, ln_on_x=False, ln_on_skip0=False):
    """The `linear` node op on the matrix cores: y = min(relu(W x + b), 20) + skips on fp32 rows; 'bf16': on bf16 rows, one MFMA per
    product, y = bf16(...) (see nbasr.h)."""
    b, c_in, ld = x.shape
    _pw_check(scheme, packed, ws, c_out, c_in, b, ld)
    scheme, s = _PW_SCHEMES[scheme], _skips3(skips)
    act, act_opt = scheme.act, scheme.act_opt
    _call(scheme.linear, act(x, 'x'), ws.data_ptr(), packed.data_ptr(), _dev(bias, 'bias'), act_opt(s[0], 'skip0'), act_opt(s[1], 'skip1'),
          act_opt(s[2], 'skip2'), act(y, 'y'), b, c_in, frames, ld, c_out, _ln(ln), int(ln_on_x), int(ln_on_skip0), _stream(x))
    return y


def _pw_projection(scheme, x, frames, packed_w_ih, b_ih, b_hh, gates_ws, hidden, ws, ln, entry=None, into=()):
    """``entry``: another entry point than the scheme's own, with ``into`` = its arguments after the pending LayerNorm."""
    b, c_in, ld = x.shape
    _pw_check(scheme, packed_w_ih, ws, 4 * hidden, c_in, b, ld)
    _call(entry or _PW_SCHEMES[scheme].projection, _PW_SCHEMES[scheme].act(x, 'x'), ws.data_ptr(), packed_w_ih.data_ptr(), _dev(b_ih, 'b_ih'),
          _dev(b_hh, 'b_hh'), _dev(gates_ws, 'gates_ws'), b, c_in, frames, ld, hidden, _ln(ln), *into, _stream(x))
    return gates_ws


# the public names: a body with its scheme bound, under the body's words (the two projections differ in their arguments: below)
pack_pointwise_weights, pack_pointwise_weights_bf16 = functools.partial(_pw_pack, 'f16x2'), functools.partial(_pw_pack, 'bf16')
pointwise_workspace, pointwise_bf16_workspace = functools.partial(_pw_workspace, 'f16x2'), functools.partial(_pw_workspace, 'bf16')
linear_fused_packed, linear_fused_bf16 = functools.partial(_pw_linear, 'f16x2'), functools.partial(_pw_linear, 'bf16')
_check_pointwise, _check_pointwise_bf16 = functools.partial(_pw_check, 'f16x2'), functools.partial(_pw_check, 'bf16')
for _bound in (pack_pointwise_weights, pack_pointwise_weights_bf16, pointwise_workspace, pointwise_bf16_workspace, linear_fused_packed, linear_fused_bf16):
    _bound.__doc__ = _bound.func.__doc__


def lstm_input_projection_packed(x, frames, packed_w_ih, b_ih, b_hh, gates_ws, hidden, ws, ln=None, batch_total=None, batch_offset=0):
    """``batch_total``: gates_ws is the (frames, batch_total, 4 hidden) gate tensor of SEVERAL forwards and this call fills utterances
    batch_offset .. batch_offset + batch - 1 of it (one recurrence over all of them follows: nbasr.h)."""
    if batch_total is None:
        return _pw_projection('f16x2', x, frames, packed_w_ih, b_ih, b_hh, gates_ws, hidden, ws, ln)
    if gates_ws.numel() < frames * batch_total * 4 * hidden:
        raise HipError(f'lstm_input_projection_packed: gates_ws holds {gates_ws.numel()} floats, ({frames}, {batch_total}, {4 * hidden}) needs more')
    return _pw_projection('f16x2', x, frames, packed_w_ih, b_ih, b_hh, gates_ws, hidden, ws, ln, 'nbasr_lstm_input_projection_packed_into',
                          (batch_total, batch_offset))


def lstm_input_projection_bf16(x, frames, packed_w_ih, b_ih, b_hh, gates_ws, hidden, ws, ln=None):
    """gates (frames, batch, 4 hidden) fp32 from the bf16 encoder output x (batch, c_in, ld), its pending LayerNorm applied on the way."""
    return _pw_projection('bf16', x, frames, packed_w_ih, b_ih, b_hh, gates_ws, hidden, ws, ln)


def linear_head(h, weight, bias, logits):
    classes, features = weight.shape
    rows = h.numel() // features
    _call('nbasr_linear_head', _dev(h, 'h'), _dev(weight, 'weight'), _dev(bias, 'bias'), _dev(logits, 'logits'), rows, features, classes, _stream(h))
    return logits


def linear_head_bct(x, frames, weight, bias, logits, ln=None):
    b, features, ld = x.shape
    classes = weight.shape[0]
    _call('nbasr_linear_head_bct', _dev(x, 'x'), _dev(weight, 'weight'), _dev(bias, 'bias'), _dev(logits, 'logits'), b, features, frames, ld,
          classes, _ln(ln), _stream(x))
    return logits
