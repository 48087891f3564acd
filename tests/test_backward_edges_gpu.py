"""Each backward kernel of csrc/backward.hip on its own, through ``nb_asr_amd.hip``, at the smallest shapes where its loops take their
second trip or a guard cuts a partly filled block -- against float64.

test_backward_gpu.py and test_model_gpu.py run these kernels at a handful of tiny shapes (LayerNorm: <= 2 tiles, relu/clamp: one trip of
the grid-stride loop, LSTM: one block of utterances, most wgrad templates: one 64-frame step), through compositions whose tolerance
would hide a dropped frame in a small-gradient channel.  Here every kernel gets explicit saved tensors, so the reference is exact linear
algebra without mask flips: ``z`` / ``y`` are built on the host from values in (-5, 25) passed through clamp(0, 20) -- both masks active
-- and the reference takes ``gm = dz * [0 < z < 20]`` from that same ``z``; the rest is float64 torch / numpy on the CPU.  Pitch columns
follow include/nbasr.h: zeros in dz / dy, a finite sentinel (7.0) in x where the header lets the caller leave anything, and exact zeros
in every output's pitch columns.

Tolerance.  Error = max|got - fp64| / max|fp64| per output tensor.  The same formulas are also evaluated in float32 on the CPU (ATen);
the bound is 4 x that evaluation's own distance to fp64 (the kernels sum in another order -- the front-end test grants 3 for the same
reason, the wgrad reduces over B x T on the matrix cores in 64-frame steps), with a floor for the cases where the CPU's error happens to
be ~0, and never looser than what test_backward_gpu.py grants (1e-4 of scale; 2e-4 for the LayerNorm's dx).  The floor is the worst
error of any kernel of this file measured once on the MI355X, rounded up to one significant digit (profiles/backward/edges_errors.json):

    FLOOR = 5e-7   (worst: 4.868e-07, the weight gradient of CG = 12, k = 7, d = 2 at T = 257; fp32 on the CPU there: 9.5e-08)
    worst measured error per kernel and output, with the fp32 CPU evaluation's error in the same case:
        layernorm            dx 1.788e-07 (2.022e-07)   dgamma 1.182e-07 (9.949e-08)   dbeta 9.515e-08 (2.728e-07)
        grouped_dgrad        dx 3.171e-07 (1.191e-07)
        grouped_wgrad        dw 4.868e-07 (9.544e-08)   db 3.182e-07 (6.230e-08)
        lstm_gate_scan       acts 8.699e-08 (8.699e-08) cells 1.089e-07 (9.893e-08)
        lstm_backward_step   dpre 1.008e-07 (5.022e-08) dc 1.459e-07 (1.319e-07)
        pointwise_linear     y 3.102e-07 (6.055e-07)    dx 2.938e-07 (2.938e-07)   dw 1.731e-07 (4.298e-07)   db 7.709e-08 (1.229e-07)
        (test_chain_replay_gpu.py, the chained backward step at H = 8: dpre 1.170e-07, dc 1.016e-07)

The index-shuffling kernels (conv_cols, rows_of_channels, zero_stuff), the relu / clamp mask and the skip sum compare exactly.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from nb_asr_amd import autograd as nb_autograd, hip

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SENTINEL = 7.0
FLOOR = 5e-7
CAP, CAP_LN_DX = 1e-4, 2e-4                                   # what test_backward_gpu.py grants


def rel_err(got, want64):
    """max|got - want| / max|want| (want all zero: the absolute error, which must then be 0 to pass any bound)."""
    got, want64 = got.detach().double().cpu(), want64.detach().double().cpu()
    assert tuple(got.shape) == tuple(want64.shape), (tuple(got.shape), tuple(want64.shape))
    scale = float(want64.abs().max()) if want64.numel() else 0.0
    err = float((got - want64).abs().max()) if want64.numel() else 0.0
    return err / scale if scale > 0 else err


def check(kernel, case, what, got, want64, want32, cap=CAP):
    """The tolerance rule of the module docstring; prints every figure before it asserts."""
    assert torch.isfinite(got).all(), f'{kernel} {case} {what}: non-finite output'
    e_gpu, e_cpu = rel_err(got, want64), rel_err(want32, want64)
    bound = min(max(4.0 * e_cpu, FLOOR), cap)
    print(f'EDGE-ERR {kernel} | {case} | {what} | gpu {e_gpu:.3e} | cpu32 {e_cpu:.3e} | bound {bound:.3e}')
    assert e_gpu <= bound, f'{kernel} {case} {what}: error {e_gpu:.3e} > bound {bound:.3e} (fp32 on the CPU: {e_cpu:.3e})'


def pitched(t, ld, fill=0.0):
    """(B, C, T) -> (B, C, ld) with the pitch columns set to ``fill``."""
    out = torch.full(t.shape[:2] + (ld,), fill, dtype=t.dtype)
    out[:, :, :t.shape[2]] = t
    return out


def masked_output(gen, shape):
    """A saved op output: values in (-5, 25) through clamp(0, 20), so both the ReLU and the clamp mask are active."""
    z = (torch.rand(shape, generator=gen) * 30.0 - 5.0).clamp(0.0, 20.0)
    flat = z.view(-1)
    flat[0], flat[flat.numel() // 2], flat[-1] = 0.0, 20.0, 10.0           # (the smallest cases need not draw all three)
    assert bool((z == 0).any()) and bool((z == 20).any()) and bool(((z > 0) & (z < 20)).any())
    return z


# ---- LayerNorm backward ------------------------------------------------------------------------------------------------------------
def layernorm_ref(x, gamma, beta, dy, eps, dtype):
    xr, gr, br = (v.to(dtype).clone().requires_grad_(True) for v in (x, gamma, beta))
    y = F.layer_norm(xr.permute(0, 2, 1), (x.shape[1],), gr, br, eps).permute(0, 2, 1)
    (y * dy.to(dtype)).sum().backward()
    return xr.grad, gr.grad, br.grad


@pytest.mark.parametrize('c,b,t', [(24, 1, 1), (40, 3, 64), (40, 3, 65), (72, 5, 257), (136, 17, 61), (600, 2, 19)])
def test_layernorm_backward_tiles(c, b, t):
    """tiles = B * ceil(ld / 64): 1, 3, 6, 25 (the reduce kernel's 4 x unrolled main loop needs >= 13), 17, 2; blockIdx.x > 0 from T = 65."""
    gen = torch.Generator().manual_seed(1000 * c + 10 * b + t)
    eps, ld = 1e-3, hip.round_up4(t)
    x = torch.randn(b, c, t, generator=gen) * 2.0 + 0.5
    gamma, beta = torch.randn(c, generator=gen) * 0.5 + 1.0, torch.randn(c, generator=gen) * 0.2
    dy = torch.randn(b, c, t, generator=gen)
    want64, want32 = layernorm_ref(x, gamma, beta, dy, eps, torch.float64), layernorm_ref(x, gamma, beta, dy, eps, torch.float32)
    xp, dyp = pitched(x, ld, SENTINEL).to(DEV), pitched(dy, ld).to(DEV)
    runs = []
    for _ in range(2):
        stats = torch.full((b, 2, ld), float('nan'), device=DEV)
        hip.channel_stats(xp, stats, t, eps)
        runs.append(hip.layernorm_channels_backward(xp, stats, gamma.to(DEV), dyp, t))
    dx, dgamma, dbeta = runs[0]
    assert all(torch.equal(u, v) for u, v in zip(*runs))                      # fixed summation order: bit-reproducible
    assert torch.equal(dx[:, :, t:], torch.zeros_like(dx[:, :, t:]))
    case = f'c{c}_b{b}_t{t}'
    check('layernorm', case, 'dx', dx[:, :, :t], want64[0], want32[0], CAP_LN_DX)
    check('layernorm', case, 'dgamma', dgamma, want64[1], want32[1])
    check('layernorm', case, 'dbeta', dbeta, want64[2], want32[2])


# ---- grouped node op: wgrad (fp32 MFMA, 64-frame steps) and dgrad (256-frame lane blocks) ----------------------------------------------
def grouped_ref(x, w, z, dz, groups, k, d, dtype):
    """gm = dz * [0 < z < 20] from the saved output; dx, dw through ATen's conv1d autograd, db = sum gm."""
    lpad, rpad = hip.pad_amounts(k, d, 1)
    xr, wr = x.to(dtype).clone().requires_grad_(True), w.to(dtype).clone().requires_grad_(True)
    gm = dz.to(dtype) * ((z > 0) & (z < 20)).to(dtype)
    y = F.conv1d(F.pad(xr, (lpad, rpad)), wr, None, 1, 0, d, groups)
    assert y.shape == gm.shape
    (y * gm).sum().backward()
    return xr.grad, wr.grad, gm.sum((0, 2))


def run_grouped(cg, k, d, groups, b, t, both_halves=False):
    gen = torch.Generator().manual_seed(((cg * 10 + k) * 10 + d) * 1000 + t)
    c, ld = cg * groups, hip.round_up4(t)
    x = torch.randn(b, c, t, generator=gen) * 2.0
    w = torch.randn(c, cg, k, generator=gen) * 0.3
    z = masked_output(gen, (b, c, t))
    dz = torch.randn(b, c, t, generator=gen)
    want64, want32 = grouped_ref(x, w, z, dz, groups, k, d, torch.float64), grouped_ref(x, w, z, dz, groups, k, d, torch.float32)
    xp, zp, dzp, wd = pitched(x, ld, SENTINEL).to(DEV), pitched(z, ld).to(DEV), pitched(dz, ld).to(DEV), w.to(DEV)
    dx, dw, db = hip.grouped_conv1d_backward(xp, wd, zp, dzp, t, groups, k, d)
    assert torch.equal(dx[:, :, t:], torch.zeros_like(dx[:, :, t:]))
    case = f'cg{cg}_k{k}_d{d}_g{groups}_b{b}_t{t}'
    check('grouped_dgrad', case, 'dx', dx[:, :, :t], want64[0], want32[0])
    check('grouped_wgrad', case, 'dw', dw, want64[1], want32[1])
    check('grouped_wgrad', case, 'db', db, want64[2], want32[2])
    if both_halves:                                           # each half alone: the same bits, and nothing for the half not asked for
        dx1, dw1, db1 = hip.grouped_conv1d_backward(xp, wd, zp, dzp, t, groups, k, d, need_dx=False)
        assert dx1 is None and torch.equal(dw1, dw) and torch.equal(db1, db)
        dx2, dw2, db2 = hip.grouped_conv1d_backward(xp, wd, zp, dzp, t, groups, k, d, need_dw=False)
        assert dw2 is None and db2 is None and torch.equal(dx2, dx)


WGRAD_TEMPLATES = [(cg, k, d) for cg in (6, 8, 10, 12) for k, d in ((5, 1), (5, 2), (7, 1), (7, 2))]


@pytest.mark.parametrize('t', [1, 63, 64, 65, 130])
@pytest.mark.parametrize('cg,k,d', WGRAD_TEMPLATES)
def test_grouped_wgrad_every_template_across_the_64_frame_step(cg, k, d, t):
    """All 16 templates below, at and beyond one 64-frame step (T = 130: three steps, the interior fast path on the far side of a step);
    groups = 3 / 5: the fourth wave of a workgroup / three waves of the second one leave at the ``g >= groups`` guard."""
    groups = 3 if (cg // 2 + k + d) % 2 else 5
    run_grouped(cg, k, d, groups, 2, t, both_halves=(t == 65))


@pytest.mark.parametrize('t', [255, 256, 257, 260])
@pytest.mark.parametrize('cg,k,d,groups', [(6, 5, 1, 5), (12, 7, 2, 3)])
def test_grouped_dgrad_across_the_256_frame_lane_block(cg, k, d, groups, t):
    run_grouped(cg, k, d, groups, 2, t, both_halves=(t == 257))


# ---- relu / clamp mask ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [16, 4 * (4096 * 256) + 4 * 257])
def test_relu_clamp_backward_mask_and_grid_stride(n):
    """The gradient passes only where 0 < y < 20 (csrc/backward.hip): not at exactly 0.0, -0.0 or 20.0, not where y is NaN.  The grid is
    capped at 4096 x 256 float4: the larger n puts 257 float4 into the second trip of the grid-stride loop."""
    gen = torch.Generator().manual_seed(n)
    y = (torch.rand(n, generator=gen) * 30.0 - 5.0).clamp(0.0, 20.0)
    dy = torch.randn(n, generator=gen)
    dy[dy == 0] = 1.0
    special = [0.0, 20.0, -0.0, float('nan'), 19.999998092651367, 10.0]       # (19.999998...: the fp32 below 20)
    for base in sorted({0, n - 8}):                           # the first float4s and the last two (the second trip, where there is one)
        for i, v in enumerate(special):
            y[base + i] = v
    want = torch.where((y > 0) & (y < 20), dy, torch.zeros_like(dy))
    assert want[n - 8: n - 2].ne(0).tolist() == [False, False, False, False, True, True]
    dz = torch.full((n,), float('nan'), device=DEV)
    hip.relu_clamp_backward(y.to(DEV), dy.to(DEV), dz)
    got = dz.cpu()
    assert torch.equal(got, want), f'{int((got != want).sum())} of {n} differ, first at {int((got != want).nonzero()[0])}'


# ---- the operand layouts of the GEMM-shaped passes: exact ---------------------------------------------------------------------------------
@pytest.mark.parametrize('t', [1, 5, 64, 65])
@pytest.mark.parametrize('c_in,taps,stride', [(5, 8, 1), (5, 8, 2), (33, 8, 2), (33, 8, 1), (6, 1, 1)])
def test_conv_cols_against_index_loops(c_in, taps, stride, t):
    """cols[b * t_pad + t'][ci * taps + j] = xpad[b][ci][t' * stride + j - lpad], a column of ones, zeros up to ld_cols (c_in * taps + 1 is
    no multiple of 4) and in the rows t' >= frames_out (t_pad > frames_out); 33 * 8 + 1 columns: a second block along x."""
    gen = torch.Generator().manual_seed(c_in * 100 + stride * 10 + t)
    b = 2
    t_out = (t + stride - 1) // stride
    t_pad, ld_in = hip.round_up4(t_out) + 4, hip.round_up4(t) + 4
    lpad = hip.pad_amounts(taps, 1, stride)[0]
    ncols = c_in * taps
    ld_cols = hip.round_up4(ncols + 1)
    assert (ncols + 1) % 4 and t_pad > t_out
    x = torch.randn(b, c_in, t, generator=gen)
    want = np.zeros((b * t_pad, ld_cols), dtype=np.float32)
    xn = x.numpy()
    for bi in range(b):
        for to in range(t_out):
            for j in range(taps):
                u = to * stride + j - lpad
                if 0 <= u < t:
                    want[bi * t_pad + to, j:ncols:taps] = xn[bi, :, u]
            want[bi * t_pad + to, ncols] = 1.0
    cols = torch.full((1, b * t_pad, ld_cols), float('nan'), device=DEV)
    hip.conv_cols(pitched(x, ld_in, SENTINEL).to(DEV), cols, t, t_out, t_pad, taps, stride, lpad)
    assert np.array_equal(cols[0].cpu().numpy(), want)


@pytest.mark.parametrize('t', [1, 5, 64, 65, 257])
def test_rows_of_channels_against_index_loops(t):
    """rows[co][b * t_pad + t'] = dz[b][co][t'], 0 for t' >= frames -- also beyond dz's own pitch (t_pad > ld); T = 257: a second block."""
    gen = torch.Generator().manual_seed(t)
    b, c = 3, 5
    ld, t_pad = hip.round_up4(t), hip.round_up4(t) + 8
    dz = torch.randn(b, c, t, generator=gen)
    want = np.zeros((c, b * t_pad), dtype=np.float32)
    for bi in range(b):
        for co in range(c):
            want[co, bi * t_pad: bi * t_pad + t] = dz[bi, co].numpy()
    rows = torch.full((c, b * t_pad), float('nan'), device=DEV)
    hip.rows_of_channels(pitched(dz, ld).to(DEV), rows, t, t_pad)
    assert np.array_equal(rows.cpu().numpy(), want)


@pytest.mark.parametrize('b,c,t,stride,shift,cut', [(1, 3, 1, 1, 0, 0), (2, 3, 5, 2, 0, 0), (2, 3, 64, 2, 1, 0), (1, 2, 65, 2, 3, 1), (2, 3, 65, 1, 2, 0),
                                                    (2, 2050, 6, 2, 1, 1)])
def test_zero_stuff_against_index_loops(b, c, t, stride, shift, cut):
    """up[r][shift + t' * stride] = dz[r][t'], zeros elsewhere; ``cut``: frames_up ends before the last stuffed frame.  The last case has
    4100 rows: the grid is capped at 4096 rows, four of them are a second trip of the row loop."""
    gen = torch.Generator().manual_seed(b * 7 + c + t + shift)
    ld = hip.round_up4(t)
    frames_up = shift + (t - 1) * stride + 1 + (2 if not cut else -1)
    ld_up = hip.round_up4(frames_up) + 4
    dz = torch.randn(b, c, t, generator=gen)
    want = np.zeros((b, c, ld_up), dtype=np.float32)
    for to in range(t):
        u = shift + to * stride
        if u < frames_up:
            want[:, :, u] = dz[:, :, to].numpy()
    up = torch.full((b, c, ld_up), float('nan'), device=DEV)
    hip.zero_stuff(pitched(dz, ld).to(DEV), up, t, frames_up, stride, shift)
    assert np.array_equal(up.cpu().numpy(), want)


# ---- LSTM: the forward scan that restores the cell states, and the reverse step -----------------------------------------------------------
def lstm_scan_ref(pre, dtype):
    """pre (4H, T, B) -> gate activations (4H, T, B) in PyTorch's order i, f, g, o and the cell states (H, T, B)."""
    pre = pre.to(dtype)
    hidden, frames = pre.shape[0] // 4, pre.shape[1]
    i, f, g, o = (torch.sigmoid(pre[:hidden]), torch.sigmoid(pre[hidden:2 * hidden]), torch.tanh(pre[2 * hidden:3 * hidden]),
                  torch.sigmoid(pre[3 * hidden:]))
    cells = torch.empty(hidden, frames, pre.shape[2], dtype=dtype)
    c = torch.zeros(hidden, pre.shape[2], dtype=dtype)
    for t in range(frames):
        c = f[:, t] * c + i[:, t] * g[:, t]
        cells[:, t] = c
    return torch.cat([i, f, g, o]), cells


def lstm_bptt_ref(dh_out, w_hh_t, dc0, acts, cells, dtype):
    """The reverse recurrence of lstm_backward_step_kernel's header comment, frames T-1 .. 0: dh_out (H, T, B), w_hh_t (H, 4H),
    dc0 (H, B) the incoming carry, acts (4H, T, B), cells (H, T, B) -> dpre (4H, T, B), the final carry (H, B)."""
    dh_out, w, dc, acts, cells = (v.to(dtype) for v in (dh_out, w_hh_t, dc0, acts, cells))
    hidden, frames, batch = cells.shape
    i, f, g, o = acts[:hidden], acts[hidden:2 * hidden], acts[2 * hidden:3 * hidden], acts[3 * hidden:]
    dpre = torch.zeros(4 * hidden, frames, batch, dtype=dtype)
    for t in range(frames - 1, -1, -1):
        gh = dh_out[:, t] + (w @ dpre[:, t + 1] if t + 1 < frames else 0.0)
        c_prev = cells[:, t - 1] if t > 0 else torch.zeros_like(cells[:, 0])
        tc = torch.tanh(cells[:, t])
        d_o = gh * tc
        d_c = dc + gh * o[:, t] * (1.0 - tc * tc)
        dpre[:hidden, t] = d_c * g[:, t] * i[:, t] * (1.0 - i[:, t])
        dpre[hidden:2 * hidden, t] = d_c * c_prev * f[:, t] * (1.0 - f[:, t])
        dpre[2 * hidden:3 * hidden, t] = d_c * i[:, t] * (1.0 - g[:, t] * g[:, t])
        dpre[3 * hidden:, t] = d_o * o[:, t] * (1.0 - o[:, t])
        dc = d_c * f[:, t]
    return dpre, dc


def batch_pitched(t, ldb, fill=0.0):
    """(rows, T, B) -> (rows, T, ldb): the utterances are innermost in the BPTT layout."""
    out = torch.full(t.shape[:2] + (ldb,), fill, dtype=t.dtype)
    out[:, :, :t.shape[2]] = t
    return out


LSTM_SHAPES = [(4, 3, 66), (8, 2, 64), (36, 5, 65), (500, 2, 3)]          # B > 64: a second, partly filled block of utterances


@pytest.mark.parametrize('hidden,frames,batch', LSTM_SHAPES)
def test_lstm_gate_scan(hidden, frames, batch):
    gen = torch.Generator().manual_seed(hidden * 100 + batch)
    ldb = hip.round_up4(batch)
    pre = torch.randn(4 * hidden, frames, batch, generator=gen) * 1.5
    (a64, c64), (a32, c32) = lstm_scan_ref(pre, torch.float64), lstm_scan_ref(pre, torch.float32)
    acts = batch_pitched(pre, ldb, SENTINEL).to(DEV)
    cells = torch.full((hidden, frames, ldb), SENTINEL, device=DEV)
    hip.lstm_gate_scan(acts, cells, batch)
    case = f'h{hidden}_t{frames}_b{batch}'
    check('lstm_gate_scan', case, 'acts', acts[:, :, :batch], a64, a32)
    check('lstm_gate_scan', case, 'cells', cells[:, :, :batch], c64, c32)
    # the pitch utterances are not the scan's to touch
    assert bool((acts[:, :, batch:] == SENTINEL).all()) and bool((cells[:, :, batch:] == SENTINEL).all())


@pytest.mark.parametrize('hidden,frames,batch', LSTM_SHAPES)
def test_lstm_backward_step_per_frame(hidden, frames, batch):
    gen = torch.Generator().manual_seed(hidden * 100 + batch + 1)
    ldb = hip.round_up4(batch)
    acts, cells = lstm_scan_ref(torch.randn(4 * hidden, frames, batch, generator=gen) * 1.5, torch.float32)      # the saved tensors
    dh_out = torch.randn(hidden, frames, batch, generator=gen)
    w_hh_t = torch.randn(hidden, 4 * hidden, generator=gen) * (0.5 / hidden ** 0.5)
    dc0 = torch.randn(hidden, batch, generator=gen) * 0.5
    (p64, d64), (p32, d32) = lstm_bptt_ref(dh_out, w_hh_t, dc0, acts, cells, torch.float64), lstm_bptt_ref(dh_out, w_hh_t, dc0, acts, cells, torch.float32)
    dc = torch.full((hidden, ldb), SENTINEL)
    dc[:, :batch] = dc0
    dc = dc.to(DEV)
    dpre = torch.full((4 * hidden, frames, ldb), float('nan'), device=DEV)
    args = (batch_pitched(dh_out, ldb).to(DEV), w_hh_t.to(DEV), dc, batch_pitched(acts, ldb, SENTINEL).to(DEV), batch_pitched(cells, ldb, SENTINEL).to(DEV), dpre)
    for t in range(frames - 1, -1, -1):
        hip.lstm_backward_step(*args, batch, t)
    case = f'h{hidden}_t{frames}_b{batch}'
    assert torch.equal(dpre[:, :, batch:], torch.zeros_like(dpre[:, :, batch:]))        # the GEMMs behind read them
    assert bool((dc[:, batch:] == SENTINEL).all())
    check('lstm_backward_step', case, 'dpre', dpre[:, :, :batch], p64, p32)
    check('lstm_backward_step', case, 'dc', dc[:, :batch], d64, d32)


# ---- the head's autograd function and the node sum ---------------------------------------------------------------------------------------
def head_ref(x, w, bias, r, dtype):
    x, w, bias, r = (v.to(dtype) for v in (x, w, bias, r))
    y = torch.einsum('oc,bct->bot', w, x) + bias.view(1, -1, 1)
    return y, torch.einsum('oc,bot->bct', w, r), torch.einsum('bot,bct->oc', r, x), r.sum((0, 2))


@pytest.mark.parametrize('b,c_in,t', [(2, 20, 7), (3, 500, 33)])
@pytest.mark.parametrize('c_out', [49, 3, 52])
def test_pointwise_linear_autograd(c_out, b, c_in, t):
    """autograd.pointwise_linear pads the class dimension to a multiple of 4 rows for its GEMMs (49 -> 52, 3 -> 4): the padding must not
    reach dW / db, whose shapes are the parameters'."""
    gen = torch.Generator().manual_seed(c_out * 1000 + c_in + t)
    x = torch.randn(b, c_in, t, generator=gen) * 2.0
    w, bias = torch.randn(c_out, c_in, generator=gen) * (1.0 / c_in ** 0.5), torch.randn(c_out, generator=gen) * 0.2
    r = torch.randn(b, c_out, t, generator=gen)
    want64, want32 = head_ref(x, w, bias, r, torch.float64), head_ref(x, w, bias, r, torch.float32)
    xg, wg, bg = (v.to(DEV).requires_grad_(True) for v in (x, w, bias))
    y = nb_autograd.pointwise_linear(xg, wg, bg)
    (y * r.to(DEV)).sum().backward()
    assert tuple(wg.grad.shape) == (c_out, c_in) and tuple(bg.grad.shape) == (c_out,) and tuple(xg.grad.shape) == (b, c_in, t)
    case = f'o{c_out}_b{b}_c{c_in}_t{t}'
    for what, got, w64, w32 in zip(('y', 'dx', 'dw', 'db'), (y, xg.grad, wg.grad, bg.grad), want64, want32):
        check('pointwise_linear', case, what, got, w64, w32)


@pytest.mark.parametrize('t', [37, 64])
@pytest.mark.parametrize('n', [2, 3, 4, 5])
def test_skip_sum_autograd(n, t):
    """Three tensors per launch, left to right: 4 and 5 terms take a second launch on the running sum.  fp32 additions in that order are
    what ATen does on the CPU: bit for bit; every term's gradient is the incoming one."""
    gen = torch.Generator().manual_seed(10 * n + t)
    terms = [torch.randn(2, 24, t, generator=gen) * 10.0 ** (i - 2) for i in range(n)]
    r = torch.randn(2, 24, t, generator=gen)
    want = terms[0]
    for term in terms[1:]:
        want = want + term
    on_dev = [v.to(DEV).requires_grad_(True) for v in terms]
    y = nb_autograd.skip_sum(on_dev)
    assert torch.equal(y.detach().cpu(), want)
    (y * r.to(DEV)).sum().backward()
    for v in on_dev:
        assert torch.equal(v.grad.cpu(), r)
