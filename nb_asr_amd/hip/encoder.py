"""The encoder's entry points: node ops, fused cells, statistics and LayerNorm, operand images, dense convolutions, stream windows.  Activations
are (batch, channels, ld) tensors whose last dimension is the row pitch ld (``row_pitch``) and `frames` <= ld the number of valid frames;
float32, or bfloat16 where a wrapper says so (SURVEY 8 row g1 / BASELINE config 4)."""
import ctypes

import torch

from . import (SIGNATURES, HipError, load_library, _call, _scratch, _opaque, _stream, _dev, _opt, _act, _act_opt, _ln, _skips3, dtype_code,
               BF16, _c_float_p, _c_int, _c_stream, _c_ln_p)

SIGNATURES.update({
    # LayerNorm, statistics, node ops (storage-type generic: a trailing dtype code)
    'nbasr_layernorm_channels': (_c_int, [_c_float_p] * 5 + [_c_int] * 4 + [ctypes.c_float, _c_int, _c_int, _c_stream]),
    'nbasr_channel_stats': (_c_int, [_c_float_p] * 2 + [_c_int] * 4 + [ctypes.c_float, _c_int, _c_stream]),
    'nbasr_grouped_stats_workspace_bytes': (ctypes.c_size_t, [_c_int] * 3),
    'nbasr_grouped_stats_finalize': (_c_int, [_c_float_p] * 2 + [_c_int] * 6 + [ctypes.c_float, _c_stream]),
    'nbasr_grouped_conv1d_node': (_c_int, [_c_float_p] * 7 + [_c_int] * 7 + [_c_ln_p, _c_int, _c_int, _c_float_p, _c_int, _c_int, _c_stream]),
    'nbasr_pack_grouped_weights': (_c_int, [_c_float_p] * 2 + [_c_int] * 3 + [_c_stream]),
    'nbasr_grouped_cell_fits': (_c_int, [_c_int] * 3),
    'nbasr_grouped_cell_fused': (_c_int, [_c_float_p, _c_float_p, _c_float_p, _c_int, _c_int, _c_float_p, _c_float_p, _c_int, _c_int,
                                          _c_float_p, _c_float_p, _c_int, _c_int, _c_int, _c_float_p] + [_c_int] * 5 + [_c_ln_p, _c_float_p, _c_int, _c_stream]),
    'nbasr_grouped_cell_mfma_weights_bytes': (ctypes.c_size_t, [_c_int] * 3),
    'nbasr_grouped_cell_mfma_pack': (_c_int, [_c_float_p] * 2 + [_c_int] * 3 + [_c_stream]),
    'nbasr_grouped_cell_mfma_fits': (_c_int, [_c_int] * 3),
    'nbasr_grouped_cell_mfma': (_c_int, [_c_float_p, _c_float_p, _c_float_p, _c_int, _c_int, _c_float_p, _c_float_p, _c_int, _c_int,
                                         _c_float_p, _c_float_p, _c_int, _c_int, _c_int, _c_float_p] + [_c_int] * 5 + [_c_ln_p, _c_stream]),
    'nbasr_skip_sum': (_c_int, [_c_float_p] * 4 + [_c_int] * 4 + [_c_ln_p, _c_int, _c_int, _c_stream]),
    'nbasr_repitch': (_c_int, [_c_float_p] * 2 + [_c_int] * 5 + [_c_stream]),
    'nbasr_convert': (_c_int, [_c_float_p] * 2 + [ctypes.c_longlong, _c_int, _c_int, _c_stream]),
    # dense convolutions
    'nbasr_dense_conv1d_fused': (_c_int, [_c_float_p] * 7 + [_c_int] * 8 + [_c_ln_p, _c_int, _c_int, _c_stream]),
    'nbasr_packed_dense_weights_bytes': (ctypes.c_size_t, [_c_int] * 5),
    'nbasr_pack_dense_weights': (_c_int, [_c_int] + [_c_float_p] * 2 + [_c_int] * 5 + [_c_stream]),
    'nbasr_dense_conv1d_packed': (_c_int, [_c_int, _c_float_p, _c_int] + [_c_float_p] * 8 + [_c_int] * 10 + [_c_ln_p, _c_float_p, _c_stream]),
    'nbasr_input_range': (_c_int, [_c_float_p] * 2 + [_c_int] * 4 + [_c_stream]),
    'nbasr_split_image_bytes': (ctypes.c_size_t, [_c_int] * 3),
    'nbasr_layernorm_split_image': (_c_int, [_c_float_p] * 6 + [_c_int] * 4 + [ctypes.c_float, _c_stream]),
    'nbasr_split_image_ranged': (_c_int, [_c_float_p] * 3 + [_c_int] * 4 + [_c_stream]),
    'nbasr_bf16_image_bytes': (ctypes.c_size_t, [_c_int] * 3),
    'nbasr_bf16_image': (_c_int, [_c_float_p] * 5 + [_c_int] * 4 + [ctypes.c_float, _c_int, _c_stream]),
    'nbasr_stream_window': (_c_int, [_c_float_p] + [_c_int] * 3 + [_c_float_p] + [_c_int] * 3 + [_c_float_p] + [_c_int] * 3 + [_c_float_p, _c_stream]),
    'nbasr_stream_window_bf16': (_c_int, [_c_float_p] + [_c_int] * 3 + [_c_float_p] + [_c_int] * 4 + [_c_float_p] + [_c_int] * 3 + [_c_stream]),
})

GC_FPL8, GC_WPERM, GC_OSPLIT, GC_PIPE, GC_RING = 1, 2, 4, 8, 16         # NBASR_GC_* variant bits of nbasr_grouped_conv1d_node
DENSE_SCHEMES = {'bf16x3': 0, 'f16x2': 1, 'bf16': 2}        # NBASR_DENSE_* of nbasr_dense_conv1d_packed
DENSE_STATS_UNIT = 16         # nbasr.h: NBASR_DENSE_STATS_UNIT


def pack_grouped_weights(weight, groups):
    """(C, C/groups, k) fp32 weight -> [group][ci][tap][co] copy for the GC_WPERM kernel variants."""
    c, cg, k = weight.shape
    packed = torch.empty_like(weight)
    _call('nbasr_pack_grouped_weights', _dev(weight, 'weight'), _dev(packed, 'packed'), c, groups, k, _stream(weight))
    return packed


def grouped_conv1d_node(x, weight, bias, skips, y, frames, groups, kernel, dilation, ln=None, ln_on_x=False, ln_on_skip0=False, stats_ws=None, variant=0):
    """The grouped-conv node op for float32 or bfloat16 activations; ``weight`` / ``bias`` are float32 (``weight`` in the
    layout the variant wants: torch's, or pack_grouped_weights' for GC_WPERM)."""
    b, c, ld = x.shape
    dt = x.dtype
    s = _skips3(skips)
    _call('nbasr_grouped_conv1d_node', _act(x, 'x'), _dev(weight, 'weight'), _dev(bias, 'bias'), _act_opt(s[0], 'skip0', dt),
          _act_opt(s[1], 'skip1', dt), _act_opt(s[2], 'skip2', dt), _act(y, 'y', dt), b, c, frames, ld, groups, kernel, dilation, _ln(ln),
          int(ln_on_x), int(ln_on_skip0), _opt(stats_ws, 'stats_ws'), dtype_code(dt), variant, _stream(x))
    return y


def grouped_conv1d_fused(x, weight, bias, skips, y, frames, groups, kernel, dilation, ln=None, ln_on_x=False,
                         ln_on_skip0=False, stats_out=None, stats_ws=None, eps=0.0):
    """The fp32 node op (the default kernel of grouped_conv1d_node).  `ln` = (stats, gamma, beta) of a pending LayerNorm carried by x
    (ln_on_x) and/or skips[0] (ln_on_skip0).  `stats_ws` (grouped_stats_workspace): also emit the partial LayerNorm statistics of y;
    with `stats_out` (B, 2, ld) they are merged at once (grouped_stats_finalize)."""
    if stats_out is not None and stats_ws is None:
        raise HipError('grouped_conv1d_fused: stats_out needs the partial-statistics workspace stats_ws')
    grouped_conv1d_node(x, weight, bias, skips, y, frames, groups, kernel, dilation, ln, ln_on_x, ln_on_skip0, stats_ws, 0)
    if stats_out is not None and x.shape[0] and x.shape[2]:
        grouped_stats_finalize(stats_ws, stats_out, x.shape[1], frames, groups, eps)
    return y


def grouped_cell_fits(channels, ld, groups):
    """0 when a (channels, ld, groups) cell cannot run as one launch, else the groups per statistics partial of that launch (4 or 2)."""
    return int(load_library().nbasr_grouped_cell_fits(channels, ld, groups))


def grouped_cell_fused(x0, nodes, skip_mask, y, frames, groups, ln=None, stats_ws=None):
    """nodes: three (weight, bias, kernel, dilation), ``weight`` = the [group][ci][tap][co] copy of ``pack_grouped_weights`` (ABI 4);
    skip_mask: bit0 s00 | bit1 s10 | bit2 s11 | bit3 s20 | bit4 s21 | bit5 s22.
    ``stats_ws`` (grouped_stats_workspace): also emit the partial LayerNorm statistics of the result (merge: grouped_stats_finalize)."""
    b, c, ld = x0.shape
    args = []
    for w, bias, k, d in nodes:
        args += [_dev(w, 'weight'), _dev(bias, 'bias'), k, d]
    dtype = x0.dtype
    _call('nbasr_grouped_cell_fused', _act(x0, 'x0', dtype), *args, skip_mask, _act(y, 'y', dtype), b, c, frames, ld, groups, _ln(ln),
          _opt(stats_ws, 'stats_ws'), dtype_code(dtype), _stream(x0))
    return y


def grouped_cell_mfma_fits(channels, ld, groups):
    """0 when a bf16 (channels, ld, groups) cell cannot run as one matrix-core launch, else its groups per workgroup."""
    return int(load_library().nbasr_grouped_cell_mfma_fits(channels, ld, groups))


def grouped_cell_mfma_pack(weight, groups):
    """(C, C/groups, k) fp32 weight (the values of a bf16 parameter) -> the MFMA fragment image grouped_cell_mfma takes for that node."""
    c, _, k = weight.shape
    nbytes = load_library().nbasr_grouped_cell_mfma_weights_bytes(c, groups, k)
    if nbytes == 0:
        raise HipError(f'grouped_cell_mfma_pack: weight shape {tuple(weight.shape)} with {groups} groups is not a node op of the search space')
    packed = torch.empty(nbytes, dtype=torch.uint8, device=weight.device)
    _call('nbasr_grouped_cell_mfma_pack', _dev(weight, 'weight'), packed.data_ptr(), c, groups, k, _stream(weight))
    return packed


def grouped_cell_mfma(x0, nodes, skip_mask, y, frames, groups, ln=None):
    """The bf16 cell on the matrix cores.  nodes: three (packed weight from grouped_cell_mfma_pack, fp32 bias, kernel, dilation)."""
    b, c, ld = x0.shape
    args = []
    for packed, bias, k, d in nodes:
        _opaque(packed, load_library().nbasr_grouped_cell_mfma_weights_bytes(c, groups, k),
                'grouped_cell_mfma: node weights must be the uint8 tensors of grouped_cell_mfma_pack for this (channels, groups, kernel)', exact=True)
        args += [packed.data_ptr(), _dev(bias, 'bias'), k, d]
    _call('nbasr_grouped_cell_mfma', _act(x0, 'x0', torch.bfloat16), *args, skip_mask, _act(y, 'y', torch.bfloat16), b, c, frames, ld, groups,
          _ln(ln), _stream(x0))
    return y


def grouped_stats_finalize(stats_ws, stats_out, channels, frames, groups, eps, groups_per_part=4):
    """Merge the partial statistics a node / fused-cell launch left in ``stats_ws`` into (mean, rstd) rows.  ``groups_per_part``: 4 for
    the node kernels, ``grouped_cell_fits(...)`` (4 or 2) for a fused cell."""
    b, _, ld = stats_out.shape
    _call('nbasr_grouped_stats_finalize', _dev(stats_ws, 'stats_ws'), _dev(stats_out, 'stats_out'), b, channels, frames, ld, groups,
          int(groups_per_part), float(eps), _stream(stats_out))
    return stats_out


def grouped_stats_workspace(batch, ld, groups, device):
    return _scratch(load_library().nbasr_grouped_stats_workspace_bytes(batch, ld, groups), device, torch.float32, 16)


def skip_sum(skips, y, frames, ln=None, ln_on_skip0=False):
    """Node whose main op is `zero`: y = sum of the skips (float32 or bfloat16 tensors, all of y's type)."""
    b, c, ld = y.shape
    dt = y.dtype
    s = _skips3(skips)
    _call('nbasr_skip_sum', _act_opt(s[0], 'skip0', dt), _act_opt(s[1], 'skip1', dt), _act_opt(s[2], 'skip2', dt), _act(y, 'y'), b, c, frames,
          ld, _ln(ln), int(ln_on_skip0), dtype_code(dt), _stream(y))
    return y


def channel_stats(x, stats, frames, eps):
    """One read pass over x (B, C, ld), float32 or bfloat16: stats (B, 2, ld) <- per-frame (mean, 1/sqrt(var + eps)) over channels."""
    b, c, ld = x.shape
    _call('nbasr_channel_stats', _act(x, 'x'), _dev(stats, 'stats'), b, c, frames, ld, float(eps), dtype_code(x.dtype), _stream(x))
    return stats


def layernorm_channels(x, gamma, beta, y, frames, eps, absmax=None):
    """LayerNorm over channels, x -> y (float32 -> float32, bfloat16 -> bfloat16 or bfloat16 -> float32); with ``absmax`` (a (B,)
    float32 device tensor; float32 tensors only) also max|y[b]| per utterance."""
    b, c, ld = x.shape
    if absmax is not None and absmax.numel() != b:
        raise HipError('absmax must hold one float per utterance')
    _call('nbasr_layernorm_channels', _act(x, 'x'), _dev(gamma, 'gamma'), _dev(beta, 'beta'), _act(y, 'y'), _opt(absmax, 'absmax'), b, c,
          frames, ld, float(eps), dtype_code(x.dtype), dtype_code(y.dtype), _stream(x))
    return y


def split_image(batch, channels, ld, device):
    """Buffer for the pre-split fp16 image of a (batch, channels, ld) activation (layernorm_split_image)."""
    return _scratch(load_library().nbasr_split_image_bytes(batch, channels, ld), device, least=16)


def layernorm_split_image(x, gamma, beta, stats, bound, image, frames, eps):
    """LayerNorm(x) written as the fp16-split image of the dense convolution; also fills stats (B, 2, ld) and bound (B)."""
    b, c, ld = x.shape
    if image.dtype != torch.uint8 or image.numel() < load_library().nbasr_split_image_bytes(b, c, ld):
        raise HipError('image buffer too small: allocate it with split_image(batch, channels, ld, device)')
    _call('nbasr_layernorm_split_image', _dev(x, 'x'), _dev(gamma, 'gamma'), _dev(beta, 'beta'), _dev(stats, 'stats'), _dev(bound, 'bound'),
          image.data_ptr(), b, c, frames, ld, float(eps), _stream(x))
    return image


def dense_conv1d_fused_packed_f16_img(image, bound, batch, c_in, frames_in, ld_in, packed, c_out, kernel, bias, y, stride,
                                      row_tile=128, stats_part=None, frame_tile=256):
    """The fp16x2 convolution on the pre-split operand image (layernorm_split_image): LDS-DMA-only GEMM.  ``stats_part``: also emit
    the partial LayerNorm statistics of y (dense_stats_part_floats)."""
    _check_packed(packed, 'f16x2', c_out, c_in, kernel, row_tile)
    if image.numel() < load_library().nbasr_split_image_bytes(batch, c_in, ld_in):
        raise HipError('image buffer too small for (batch, c_in, ld_in)')
    return _dense_packed('f16x2', image.data_ptr(), True, bound, None, packed, bias, (None, None, None), y, _dev(y, 'y'), batch, c_in,
                         frames_in, ld_in, c_out, kernel, stride, row_tile, None, _stream(y), stats_part, frame_tile)


def input_range(x, frames, out):
    """out (B, 4) float32 <- per utterance (max finite |x|, quietest non-silent frame's max, non-finite flag, -); see nbasr.h."""
    b, c, ld = x.shape
    if out.numel() < 4 * b:
        raise HipError('input_range: out needs 4 floats per utterance')
    _call('nbasr_input_range', _dev(x, 'x'), _dev(out, 'range'), b, c, frames, ld, _stream(x))
    return out


def dense_conv1d_first_ranged(x, frames_in, x_range, packed_f16, packed_bf16x3, c_out, kernel, bias, y, stride, image=None, row_tile=128,
                              stats_part=None, frame_tile=256):
    """The model's first dense conv with per-utterance routing on the device: ordinary utterances on the 2-way fp16 split,
    extreme ones (non-finite samples, > 2^12 dynamic range between frames) on the 3-way bf16 split; same output tensor.
    ``image``: uint8 workspace of ``nbasr_split_image_bytes`` -- the fp16 leg then runs on the image path (one split pass over
    x, LDS-DMA-only GEMM; ``packed_f16`` packed for ``row_tile``); None: the input is split in the GEMM's prologue."""
    b, c_in, ld_in = x.shape
    _check_packed(packed_f16, 'f16x2', c_out, c_in, kernel, 128 if image is None else row_tile)
    _check_packed(packed_bf16x3, 'bf16x3', c_out, c_in, kernel)
    none3, stream = (None, None, None), _stream(x)
    if image is not None:
        if image.dtype != torch.uint8 or image.numel() < load_library().nbasr_split_image_bytes(b, c_in, ld_in):
            raise HipError('dense_conv1d_first_ranged: image workspace too small (nbasr_split_image_bytes)')
        _call('nbasr_split_image_ranged', _dev(x, 'x'), _dev(x_range, 'x_range'), image.data_ptr(), b, c_in, frames_in, ld_in, stream)
    x16, tile, tile_t = (_dev(x, 'x'), 128, 256) if image is None else (image.data_ptr(), row_tile, frame_tile)
    _dense_packed('f16x2', x16, image is not None, None, x_range, packed_f16, bias, none3, y, _dev(y, 'y'), b, c_in, frames_in, ld_in, c_out, kernel,
                  stride, tile, None, stream, stats_part, tile_t)
    return _dense_packed('bf16x3', _dev(x, 'x'), False, None, x_range, packed_bf16x3, bias, none3, y, _dev(y, 'y'), b, c_in, frames_in,
                         ld_in, c_out, kernel, stride, 128, None, stream, stats_part)


def dense_conv1d_fused(x, frames_in, weight, bias, skips, y, stride, ln=None, ln_on_x=False, ln_on_skip0=False):
    b, c_in, ld_in = x.shape
    c_out, _, kernel = weight.shape if weight.dim() == 3 else (weight.shape[0], weight.shape[1], 1)
    ld_out = y.shape[2]
    s = _skips3(skips)
    _call('nbasr_dense_conv1d_fused', _dev(x, 'x'), _dev(weight, 'weight'), _dev(bias, 'bias'), _opt(s[0], 'skip0'), _opt(s[1], 'skip1'), _opt(s[2], 'skip2'),
          _dev(y, 'y'), b, c_in, frames_in, ld_in, c_out, ld_out, kernel, stride, _ln(ln), int(ln_on_x), int(ln_on_skip0), _stream(x))
    return y


def _scheme_code(scheme):
    if scheme not in DENSE_SCHEMES:
        raise HipError(f"unknown operand scheme {scheme!r} (expected 'bf16x3', 'f16x2' or 'bf16')")
    return DENSE_SCHEMES[scheme]


def packed_dense_weights_bytes(scheme, c_out, c_in, kernel, row_tile=128):
    return load_library().nbasr_packed_dense_weights_bytes(_scheme_code(scheme), c_out, c_in, kernel, row_tile)


def pack_dense_weights(weight, stride, scheme='bf16x3', row_tile=128):
    """(c_out, c_in, 8) fp32 weight -> opaque uint8 tensor holding its operand form (3 x bf16 split, 2 x fp16 split for
    ``scheme='f16x2'``, one bf16 term for 'bf16') in the LDS layout of the stride-`stride` kernel that will consume it.  ``row_tile``
    other than 128: the 64- / 160-row tiles of the image-path kernels (f16x2: 64, 160; bf16: 160)."""
    code = _scheme_code(scheme)
    c_out, c_in, kernel = weight.shape
    nbytes = load_library().nbasr_packed_dense_weights_bytes(code, c_out, c_in, kernel, row_tile)
    if nbytes == 0:
        raise HipError(f'packed dense path ({scheme}) does not cover weight shape {tuple(weight.shape)} with row_tile={row_tile}')
    if not weight.is_cuda:
        raise HipError('weight must be on a HIP device')
    packed = torch.empty(nbytes, dtype=torch.uint8, device=weight.device)
    _call('nbasr_pack_dense_weights', code, _dev(weight, 'weight'), packed.data_ptr(), c_out, c_in, kernel, stride, row_tile, _stream(weight))
    packed.nbasr_row_tile = row_tile           # the packed sizes of the two tilings can coincide (c_out = 1200): remember which
    return packed


def pack_dense_weights_bf16(weight, stride, row_tile=128):
    """(c_out, c_in, 8) fp32 weight (the values of a bf16 parameter) -> packed one-term bf16 image of the stride-`stride` kernel."""
    return pack_dense_weights(weight, stride, 'bf16', row_tile)


def _dense_packed(scheme, x_ptr, image, x_absmax, x_range, packed, bias, s, y, y_ptr, b, c_in, frames_in, ld_in, c_out, kernel, stride,
                  row_tile, ln, stream, stats_part=None, frame_tile=256):
    """The one C entry point of the packed k = 8 convolution (nbasr.h: nbasr_dense_conv1d_packed)."""
    if stats_part is not None and stats_part.numel() < dense_stats_part_floats(b, c_out, y.shape[2]):
        raise HipError('stats_part too small: ceil(c_out / 16) * batch * 2 * ld_out floats (dense_stats_part_floats)')
    _call('nbasr_dense_conv1d_packed', _scheme_code(scheme), x_ptr, int(image), _opt(x_absmax, 'x_absmax'), _opt(x_range, 'x_range'),
          packed.data_ptr(), _dev(bias, 'bias'), _opt(s[0], 'skip0'), _opt(s[1], 'skip1'), _opt(s[2], 'skip2'), y_ptr, b, c_in, frames_in, ld_in,
          c_out, y.shape[2], kernel, stride, row_tile, int(frame_tile), _ln(ln), _opt(stats_part, 'stats_part'), stream)
    return y


def dense_stats_part_floats(batch, c_out, ld_out):
    """Floats of the statistics partials a dense convolution emits with ``stats_part``: one (mean, M2) row pair per 16 output channels
    (merge: grouped_stats_finalize(part, stats, c_out, frames_out, c_out, eps, DENSE_STATS_UNIT))."""
    return -(-c_out // DENSE_STATS_UNIT) * batch * 2 * ld_out


def _check_packed(packed, scheme, c_out, c_in, kernel, row_tile=128):
    if not packed.is_cuda or packed.dtype != torch.uint8:
        raise HipError('packed weights must be the uint8 device tensor returned by pack_dense_weights')
    wrong = ('packed weights have {} bytes: not a {} image of a ({}, {}, {}) weight for row_tile={}', packed.numel(), scheme, c_out, c_in, kernel, row_tile)
    if getattr(packed, 'nbasr_row_tile', 128) != row_tile:
        raise HipError(wrong[0].format(*wrong[1:]))
    _opaque(packed, packed_dense_weights_bytes(scheme, c_out, c_in, kernel, row_tile), wrong, exact=True)


def dense_conv1d_fused_packed(x, frames_in, packed, c_out, kernel, bias, skips, y, stride, ln=None, scheme='bf16x3', x_absmax=None, stats_part=None):
    """Dense k=8 conv on packed weights; ``scheme`` must be the one the weights were packed with.  'f16x2' needs
    ``x_absmax``: a (B,) float32 device tensor of upper bounds of max|x[b]| (see nbasr.h) and takes no deferred LayerNorm.
    ``stats_part`` (no skips): also emit the partial LayerNorm statistics of y (dense_stats_part_floats)."""
    b, c_in, ld_in = x.shape
    s = _skips3(skips)
    _check_packed(packed, scheme, c_out, c_in, kernel)
    if scheme == 'f16x2':
        if ln is not None:
            raise HipError('the f16x2 scheme takes no deferred LayerNorm (it needs the range of the normalised tensor)')
        if x_absmax is None or x_absmax.numel() != b:
            raise HipError('the f16x2 scheme needs x_absmax: one float32 bound of max|x[b]| per utterance')
    elif ln is not None and any(t is not None for t in s):
        raise HipError('the packed path takes a deferred LayerNorm only without skip inputs')
    return _dense_packed(scheme, _dev(x, 'x'), False, x_absmax if scheme == 'f16x2' else None, None, packed, bias, s, y, _dev(y, 'y'),
                         b, c_in, frames_in, ld_in, c_out, kernel, stride, 128, ln, _stream(x), stats_part)


def bf16_image_bytes(batch, channels, ld):
    return load_library().nbasr_bf16_image_bytes(batch, channels, ld)


def bf16_image(x, image, frames, norm=None, stats=None, eps=0.0):
    """Operand image of the bf16 dense conv from x (B, C, ld); ``norm`` = (gamma, beta): image of LayerNorm(x), ``stats`` filled."""
    b, c, ld = x.shape
    if image.dtype != torch.uint8 or image.numel() < bf16_image_bytes(b, c, ld):
        raise HipError('image buffer too small: needs bf16_image_bytes(batch, channels, ld) bytes of uint8')
    gamma, beta = norm if norm is not None else (None, None)
    _call('nbasr_bf16_image', _act(x, 'x'), _opt(gamma, 'gamma'), _opt(beta, 'beta'), _opt(stats, 'stats'), image.data_ptr(), b, c, frames, ld,
          float(eps), dtype_code(x.dtype), _stream(x))
    return image


def dense_conv1d_bf16_img(image, batch, c_in, frames_in, ld_in, packed, c_out, kernel, bias, y, stride, row_tile=128, frame_tile=256):
    _check_packed(packed, 'bf16', c_out, c_in, kernel, row_tile)
    if image.numel() < load_library().nbasr_bf16_image_bytes(batch, c_in, ld_in):
        raise HipError('image buffer too small for (batch, c_in, ld_in)')
    return _dense_packed('bf16', image.data_ptr(), True, None, None, packed, bias, (None, None, None), y, _act(y, 'y', torch.bfloat16), batch,
                         c_in, frames_in, ld_in, c_out, kernel, stride, row_tile, None, _stream(y), None, frame_tile)


def repitch(src, dst, frames):
    """src (..., ld_src) -> dst (..., ld_dst), float32 or bfloat16: copy `frames` columns, zero the rest of dst's pitch."""
    rows = src.numel() // src.shape[-1]
    _call('nbasr_repitch', _act(src, 'src'), _act(dst, 'dst', src.dtype), rows, frames, src.shape[-1], dst.shape[-1], dtype_code(src.dtype), _stream(src))
    return dst


def convert(x, y):
    """Storage conversion float32 <-> bfloat16 of equally shaped contiguous tensors (numel % 8 == 0)."""
    if x.shape != y.shape:
        raise HipError('convert: shapes differ')
    _call('nbasr_convert', _act(x, 'x'), _act(y, 'y'), x.numel(), dtype_code(x.dtype), dtype_code(y.dtype), _stream(x))
    return y


def stream_window(hist, hist_off, n_hist, src, src_off, n_new, dst, absmax=None):
    """One stage window of a streaming session (nbasr.h: nbasr_stream_window).  ``hist`` / ``src`` / ``dst``: (batch, channels, ld)
    float32 tensors with their own row pitches (``hist`` / ``src`` may be None when their frame count is 0); ``absmax`` (batch) or None."""
    b, c, dst_ld = dst.shape
    for t, what in ((hist, 'hist'), (src, 'src')):
        if t is not None and (t.shape[0] != b or t.shape[1] != c):
            raise HipError(f'stream_window: {what} has shape {tuple(t.shape)}, dst {tuple(dst.shape)}')
    if absmax is not None and absmax.numel() != b:
        raise HipError('stream_window: absmax must hold one float per utterance')
    _call('nbasr_stream_window', _opt(hist, 'hist') if n_hist else None, hist.shape[2] if hist is not None else 0, int(hist_off), int(n_hist),
          _opt(src, 'src') if n_new else None, src.shape[2] if src is not None else 0, int(src_off), int(n_new), _dev(dst, 'dst'), dst_ld, b, c,
          _opt(absmax, 'absmax'), _stream(dst))
    return dst


def stream_window_bf16(hist, hist_off, n_hist, src, src_off, n_new, dst):
    """One bfloat16 stage window of a streaming session (nbasr.h: nbasr_stream_window_bf16).  ``hist`` / ``dst``: (batch, channels, ld)
    bfloat16 tensors, ``src`` bfloat16 or float32 (rounded on the way: the front-end's frames), each with its own row pitch (``hist`` /
    ``src`` may be None when their frame count is 0); ``dst``'s pitch is a multiple of 8."""
    b, c, dst_ld = dst.shape
    for t, what in ((hist, 'hist'), (src, 'src')):
        if t is not None and (t.shape[0] != b or t.shape[1] != c):
            raise HipError(f'stream_window_bf16: {what} has shape {tuple(t.shape)}, dst {tuple(dst.shape)}')
    _call('nbasr_stream_window_bf16', _act_opt(hist, 'hist', torch.bfloat16) if n_hist else None, hist.shape[2] if hist is not None else 0,
          int(hist_off), int(n_hist), _act_opt(src, 'src', None) if n_new else None, dtype_code(src.dtype) if src is not None else BF16,
          src.shape[2] if src is not None else 0, int(src_off), int(n_new), _act(dst, 'dst', torch.bfloat16), dst_ld, b, c, _stream(dst))
    return dst
