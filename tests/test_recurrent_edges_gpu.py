"""The recurrent tail at the edges of its loops, against fp64: the fp32 recurrences (lstm.hip), the fp16-split ones (lstm_xcd.hip), the
exact-fp32 input projection (gemm_conv.hip) and the head (head_kernel).  Lists and the restatement: tests/lstm_model.py.

    A  lstm_recurrence_packed    hidden 4, 8, 12 (half a slice, a slice, a second half slice); 16 | 20 (1 -> 2 k-chunks); 64 | 68 (kchunks_p
       one axis at a time         4 -> 8, wave 1 gets work); 500; 508 | 512 (last chunk of the single round); 516 (first chunk of the second
       around H 36, B 17, T 3     round); 1024 (two full rounds).  batch 1, 15 | 16 | 17, 32 | 33 (the priority switch) at H = 36 and 500.
                                  frames 1, 2, 5 (frame 0 reads neither cell nor h).  Every utterance of B = 17 alone at H = 12, 500, 516.
    B  lstm_recurrence_seq       the hidden set up to 512, the batch set, and (B 64, H 512) = 256 workgroups: the bits of A, status clear.
    C  lstm_recurrence_xcd,      hidden 4 (one row tile; the other waves read the clamped slice), 8, 12, 16 | 20 (a second slice), 28 | 32 | 36
       _frames16, _frames16_state (a k-step; the slice >> 1 term of lx_publish_offset), 60 | 64 | 68, 500, 508 | 512.  batch as A (WPB 2 -> 4
                                  at 33).  frames 1, 2, 3, 5 (the pre_a / pre_b / pre_c rotation).  frames16 = the bits of xcd; frames16_state
                                  split after every frame of T = 5 at H = 4, 36, 500 = the bits of the unsplit run.
    D  the gate arithmetic       w_hh = 0, a (64, 512) grid of 105 values per gate (41 across each of +-[0.34, 0.36], +-0, +-1e-30, 1e-8,
                                  +-0.1 ... +-1e4): every value in every role, every (g, o) pair; all four recurrences at T = 1 and 2.  +-Inf gates saturate.
    E  lstm_input_projection     around c_in 36, H 36, T 5, B 3: c_in 4, 32 | 36, 124 | 128 | 132, 260 (K-steps, the blocked-sum flush, two);
                                  hidden 4, 32, 36, 500 (16 rows, one 128-row tile, 144, the model's); frames 1, 127 | 128 | 129; batch 1, 3;
                                  every utterance alone; with and without a deferred LayerNorm.
    F  linear_head, _bct         around rows 65, features 132, classes 49: rows 1, 15 | 16 | 17, 63 | 64 | 65; features 4, 12 | 16 | 20,
                                  124 | 128 | 132, 256 | 260, 500, 1200; classes 1, 15 | 16 | 17, 48 | 49, 63 | 64; 65 classes raise.  BCT:
                                  (B 7, T 5), (B 3, T 17) with ld > frames, with and without the deferred LayerNorm.

THE CRITERION (lstm_model.Family), one rule: truth = the fp64 restatement, want = the fp32 restatement on the CPU (for E and F the fp32 CPU
matmul on contiguous operands, as the oracle's own line has it) -- never another HIP kernel.  Against truth, got is held to cases.FACTORS:
rms error <= 1.5 x want's, per case; worst element <= 2 x want's worst over the pooled cases of one edge family (one kernel, one swept
axis).  h_out and cell_ws separately.  The fp16-split kernels get an rms floor from their documented 2-ulp functions (lstm_model.xcd_floor:
6.9e-8 for h, derived there), nothing on the worst element; no other kernel gets a floor.  Every output sits in the middle of a NaN-filled
allocation whose guards stay NaN.  D has its own bound, from the per-function accuracy alone (9 ulp of h_0, 12 of h_1: derived above
test_gate_arithmetic).  A CPU product's error depends on the routine its shape selects, so one family shares one routine: the frame
counts of E are prefixes of one 129-frame draw, the class counts of F the first columns of one 64-class product (see those tests).

MEASURED (MI355X), worst e_gpu / e_ref per kernel and family, rms (largest over the cases) | worst element (pooled); h_out, then cell_ws:
    lstm_recurrence_packed      hidden  1.12 | 0.86, 1.15 | 0.86  (rms at H = 4)    batch  1.08 | 0.61, 1.09 | 0.58    frames  1.07 | 0.97, 1.09 | 0.80
                                -- the fp32 kernel's own distance to fp64, which no test had bounded: e_gpu rms 1.2e-8 ... 2.9e-8, worst 5.0e-7 (H = 1024)
    lstm_recurrence_seq         the bits of lstm_recurrence_packed at all 22 shapes, (B 64, H 512) included; status clear
    lstm_recurrence_xcd         hidden  1.73 | 0.79, 1.31 | 0.65  (rms at H = 4)    batch  1.47 | 0.79, 1.30 | 0.88    frames  1.51 | 1.30, 1.40 | 1.01  (rms at T = 1)
                                (raw ratios, before the floor: the rms leg needs it at H = 4 and at T = 1, where the error is the functions' alone)
    lstm_recurrence_frames16    the bits of lstm_recurrence_xcd at all 30 shapes
    ..._frames16_state          split after every frame: the bits of the unsplit run; continue with h0 = None:  1.62 | 1.46 (H 4), 1.48 | 1.07 (H 36), 1.41 | 0.40 (H 500)
    gate arithmetic (ulp of h)  packed, seq: 2.35 at T = 1, 2.42 at T = 2 (the fp32 CPU restatement: 2.35, 2.45);  xcd, frames16: 2.86, 3.08; all at the
                                crossover values +-[0.34, 0.36]; bounds 9 and 12
    lstm_input_projection       1.00 | 1.00 in every family without a LayerNorm (the kernel's blocked k-ordered sum has the error of the CPU's routine to
                                three digits; 0.96 at c_in 132, 1.05 at B = 1), 0.98 ... 1.02 | 0.90 ... 1.05 with one
    linear_head                 rows  1.21 | 1.06  (rms at rows = 1)    features  1.01 | 0.71    classes  1.10 | 1.09    bct  1.03 | 1.11    bct + ln  1.03 | 1.00
60 cases, 3 s on an MI355X (the slowest, the packed batch family, 0.4 s).

FOUND BY D: lx_sigmoid multiplied by log2 e in fp32 before exp2, which loses |v| 2^-24 ln 2 of the result: 20.6 ulp of h at i = o = -30 (4.97 at
-17), where the fp32 kernels and the CPU give 2.4.  lstm_xcd.hip now hands the product's rounding on to the result (lx_exp_neg): 2.86.

Broken by hand, once each, on a scratch copy (numbers only, never an address or a wait):
    no second round in lstm_step_packed_kernel (`base < kchunks_p && base < 32`)    A hidden fails at exactly H = 516 and 1024 (rms 6.5e-3, 7.5e-2)
    `if (t > 1) c_prev = cell[...]`                                                    A fails in all three families, B at all 22 shapes (seq is intact), D packed at T = 2
    head: `part` dropped at the fold instead of added                                  F fails in all five tests (features > 128; the base has 132)
    lx_tanh: series below 3.5 instead of 0.35                                          C, the state test and D fail for xcd and frames16
    lx_tanh: series below 0.035 only                                                   NOTHING fails: the rational form costs 5.6 ulp of h at g = +-0.1 where the
        bound that follows from 2 ulp per function is 9; its error grows like 2^-24 / x and would pass 9 ulp below x ~ 0.03 -- where such a crossover
        sends nothing.  The issue's value list has nothing between 1e-8 and 0.1, and a value there could only catch shifts to below itself.
    the packers' `k < hidden` masks writing 1 instead of 0 (lstm_pack_whh_kernel, lx_pack_kernel)   NOTHING fails and nothing can: both step kernels zero h
        beyond `hidden` (`k < hidden` at the load, `live[c]`, the zeroed image rows), so those weights meet 0; the mask saves an out-of-bounds read, not a bit.
"""
import functools

import numpy as np
import pytest
import torch

import lstm_model as lm
from nb_asr_amd import hip

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F32, F64 = torch.float32, torch.float64
NAN = float('nan')
GUARD = 64                       # elements on either side of an output: 256 bytes, the output stays 16-byte aligned
EPS = 1e-3
NO_FLOOR = ((0.0, 0.0), (0.0, 0.0))


# ---- plumbing -----------------------------------------------------------------------------------------------------------------------
def guarded(shape, dtype=F32):
    """(the whole NaN-filled allocation, a contiguous view of its middle of the given shape)."""
    n = int(np.prod(shape))
    whole = torch.full((n + 2 * GUARD,), NAN, dtype=dtype, device=DEV)
    return whole, whole[GUARD:GUARD + n].view(shape)


def guards_intact(whole):
    return bool(torch.isnan(whole[:GUARD]).all()) and bool(torch.isnan(whole[-GUARD:]).all())


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@functools.lru_cache(maxsize=None)
def reference(hidden, batch, frames):
    """One draw per shape and both restatements of it, computed once: (gates, w_hh, (truth h, c), (want h, c)), all on the CPU."""
    gates, w_hh = lm.draw(hidden, batch, frames)
    return gates, w_hh, lm.recurrence(gates, w_hh, F64), lm.recurrence(gates, w_hh, F32)


def _outputs(batch, frames, hidden):
    (whole_h, h), (whole_c, cell) = guarded((batch, frames, hidden)), guarded((batch, hidden))
    return whole_h, h, whole_c, cell


def _collect(who, whole_h, h, whole_c, cell):
    torch.cuda.synchronize()
    assert guards_intact(whole_h), f'{who} wrote outside h_out'
    assert guards_intact(whole_c), f'{who} wrote outside cell_ws'
    out_h, out_c = h.cpu(), cell.cpu()
    assert bool(torch.isfinite(out_h).all()) and bool(torch.isfinite(out_c).all()), f'{who}: an element of h_out or cell_ws was not written'
    return out_h, out_c


def run_packed(gates, w_hh):
    """lstm_recurrence_packed on CPU tensors -> (h, c_T) on the CPU; fresh NaN-filled, guarded outputs."""
    t_n, b, h4 = gates.shape
    outs = _outputs(b, t_n, h4 // 4)
    hip.lstm_recurrence_packed(gates.to(DEV), hip.lstm_pack_whh(w_hh.to(DEV)), outs[3], outs[1])
    return _collect('lstm_recurrence_packed', *outs)


def run_seq(gates, w_hh):
    """lstm_recurrence_seq, or None where the device does not hold the grid (never forced)."""
    t_n, b, h4 = gates.shape
    ws = hip.lstm_seq_workspace(b, h4 // 4, DEV)
    if ws is None:
        return None
    outs = _outputs(b, t_n, h4 // 4)
    hip.lstm_recurrence_seq(gates.to(DEV), hip.lstm_pack_whh(w_hh.to(DEV)), outs[3], outs[1], ws)
    hip.lstm_seq_status(ws)
    return _collect('lstm_recurrence_seq', *outs)


def run_16(form, gates, w_hh, h0=None, c0=None, flags=0):
    """'xcd' | 'frames16' | 'state' on CPU tensors -> (h, c_T) on the CPU.  'state': c0 is put into cell_ws first (read with LSTM_CONTINUE)."""
    t_n, b, h4 = gates.shape
    hid = h4 // 4
    assert hip.lstm_xcd_workspace_bytes(b, hid) > 0
    ws, packed = hip.lstm_xcd_workspace(b, hid, DEV), hip.lstm_pack_whh16(w_hh.to(DEV))
    outs = _outputs(b, t_n, hid)
    if form == 'xcd':
        hip.lstm_recurrence_xcd(gates.to(DEV), packed, outs[3], outs[1], ws)
        hip.lstm_seq_status(ws)                                # raises if a wait timed out or a tile was never computed
    elif form == 'frames16':
        hip.lstm_recurrence_frames16(gates.to(DEV), packed, outs[3], outs[1], ws)
    else:
        if c0 is not None:
            outs[3].copy_(c0.to(DEV))
        hip.lstm_recurrence_frames16_state(gates.to(DEV), packed, outs[3], outs[1], ws, None if h0 is None else h0.contiguous().to(DEV), flags)
    return _collect(f'lstm_recurrence_{form}', *outs)


def hold(name, cases_, run, floor=lambda frames: NO_FLOOR, also=None):
    """One edge family of one recurrence kernel under the criterion, h_out and cell_ws separately; ``also(case, gates, w_hh, h, c)``:
    what else is asserted on each case."""
    fam_h, fam_c = lm.Family(f'{name} h'), lm.Family(f'{name} c')
    for hidden, batch, frames in cases_:
        gates, w_hh, (truth_h, truth_c), (want_h, want_c) = reference(hidden, batch, frames)
        h, c = run(gates, w_hh)
        case = f'H {hidden} B {batch} T {frames}'
        fam_h.add(case, h, want_h, truth_h, floor(frames)[0])
        fam_c.add(case, c, want_c, truth_c, floor(frames)[1])
        if also is not None:
            also((hidden, batch, frames), gates, w_hh, h, c)
    fam_h.close()
    fam_c.close()


# ---- A. one launch per frame, fp32 ------------------------------------------------------------------------------------------------------
SWEEPS_F32 = lm.sweeps(lm.HIDDEN_F32, lm.BATCHES, lm.FRAMES_F32)
SWEEPS_XCD = lm.sweeps(lm.HIDDEN_XCD, lm.BATCHES, lm.FRAMES_XCD)


@pytest.mark.parametrize('axis', sorted(SWEEPS_F32))
def test_packed_recurrence_vs_fp64(axis):
    hold(f'packed {axis}', SWEEPS_F32[axis], run_packed)


@pytest.mark.parametrize('hidden', lm.ALONE_HIDDEN)
def test_packed_recurrence_every_utterance_alone(hidden):
    _, batch, frames = lm.BASE
    gates, w_hh = reference(hidden, batch, frames)[:2]
    h, c = run_packed(gates, w_hh)
    for u in range(batch):
        h_u, c_u = run_packed(gates[:, u:u + 1].contiguous(), w_hh)
        assert same_bits(h_u[0], h[u]) and same_bits(c_u[0], c[u]), f'utterance {u} alone differs from the batch'


# ---- B. the one-launch fp32 form: the bits of A ---------------------------------------------------------------------------------------------
SEQ_CASES = list(dict.fromkeys([(h, b, t) for h, b, t in SWEEPS_F32['hidden'] + SWEEPS_F32['batch'] if h <= 512] + [(*lm.SEQ_RESIDENCY, lm.BASE[2])]))


@pytest.mark.parametrize('hidden,batch,frames', SEQ_CASES)
def test_seq_recurrence_is_the_bits_of_the_per_frame_one(hidden, batch, frames):
    gates, w_hh = reference(hidden, batch, frames)[:2]
    got = run_seq(gates, w_hh)                                  # (reads the status word: raises unless it is clear)
    if got is None:
        pytest.skip(f'this device does not hold the {-(-hidden // 8) * -(-batch // 16)} workgroups of the one-launch form at once')
    h, c = run_packed(gates, w_hh)
    assert same_bits(got[0], h), 'h_out differs from lstm_recurrence_packed'
    assert same_bits(got[1], c), 'cell_ws differs from lstm_recurrence_packed'


# ---- C. the fp16-split forms -------------------------------------------------------------------------------------------------------------
xcd_floor = lm.xcd_floor


def frames16_is_the_same_bits(case, gates, w_hh, h, c):
    h16, c16 = run_16('frames16', gates, w_hh)
    assert same_bits(h16, h) and same_bits(c16, c), (case, 'lstm_recurrence_frames16 differs from lstm_recurrence_xcd')


@pytest.mark.parametrize('axis', sorted(SWEEPS_XCD))
def test_xcd_recurrence_vs_fp64_and_frames16_bit_equal(axis):
    hold(f'xcd {axis}', SWEEPS_XCD[axis], functools.partial(run_16, 'xcd'), xcd_floor, frames16_is_the_same_bits)


@pytest.mark.parametrize('hidden', lm.STATE_HIDDEN)
def test_frames16_state_split_after_every_frame(hidden):
    batch, frames = 17, 5
    gates, w_hh = reference(hidden, batch, frames)[:2]
    h, c = run_16('frames16', gates, w_hh)
    plain = run_16('state', gates, w_hh)
    assert same_bits(plain[0], h) and same_bits(plain[1], c), 'flags = 0, h0 = None differs from lstm_recurrence_frames16'
    fam_h, fam_c = lm.Family(f'frames16_state H {hidden} continue, h0 = None: h'), lm.Family(f'frames16_state H {hidden} continue, h0 = None: c')
    for cut in range(1, frames):
        h1, c1 = run_16('state', gates[:cut].contiguous(), w_hh)
        assert same_bits(h1, h[:, :cut].contiguous()), cut
        h2, c2 = run_16('state', gates[cut:].contiguous(), w_hh, h0=h1[:, cut - 1], c0=c1, flags=hip.LSTM_CONTINUE)
        assert same_bits(h2, h[:, cut:].contiguous()) and same_bits(c2, c), (cut, 'the split run differs from the unsplit one')
        # LSTM_CONTINUE without h0: h_(-1) = 0, c carried
        h3, c3 = run_16('state', gates[cut:].contiguous(), w_hh, h0=None, c0=c1, flags=hip.LSTM_CONTINUE)
        truth, want = (lm.recurrence(gates[cut:], w_hh, dt, h0=None, c0=c1) for dt in (F64, F32))
        fam_h.add(f'cut {cut}', h3, want[0], truth[0], xcd_floor(frames - cut)[0])
        fam_c.add(f'cut {cut}', c3, want[1], truth[1], xcd_floor(frames - cut)[1])
    fam_h.close()
    fam_c.close()


# ---- D. the gate arithmetic, without a product ---------------------------------------------------------------------------------------------
# With w_hh = 0, h_0 = sigmoid(o) tanh(c_0), c_0 = sigmoid(i) tanh(g)  (sigmoid(f) 0 = 0 exactly), and with the same gates in frame 1
# c_1 = sigmoid(f) c_0 + sigmoid(i) tanh(g) = (1 + sigmoid(f)) c_0: two terms of one sign.  In ulp of the result (relative 2^-23 at most),
# for functions at <= 2 ulp each -- what lstm_xcd.hip documents for its exp2 / rcp forms, and what HIP documents for the expf (1 ulp, then
# 1 + e and the division rounded: 2) and tanhf (2) of lstm.hip:
#     c_0:  2 (sigmoid i) + 2 (tanh g) + 0.5 (the product)                                            = 4.5
#     h_0:  4.5 carried through tanh, whose condition number x (1 - tanh^2) / tanh is <= 1,
#           + 2 (tanh c) + 2 (sigmoid o) + 0.5 (the product)                                          = 9
#     c_1:  the term sigmoid(f) c_0 carries 2 + 4.5 + 0.5 = 7, the other 4.5; a sum of two terms of one sign carries at most the
#           larger of its terms' relative errors, + 0.5 for its own rounding                          = 7.5
#     h_1:  7.5 + 2 + 2 + 0.5                                                                         = 12
# Below |truth| = 1e-30 the sigmoid of -88 and beyond is a subnormal number, which the hardware exp2 may flush: there got is 0 or of the
# truth's sign, and below 2e-30.
GATE_BOUND_ULP = {0: 9.0, 1: 12.0}
GATE_RUNNERS = {'packed': run_packed, 'seq': run_seq, 'xcd': functools.partial(run_16, 'xcd'), 'frames16': functools.partial(run_16, 'frames16')}


@functools.lru_cache(maxsize=None)
def gate_truth(frames):
    grid = lm.gate_grid(frames)
    w_hh = torch.zeros(4 * lm.GATE_GRID[1], lm.GATE_GRID[1])
    return grid, w_hh, lm.recurrence(grid, w_hh, F64)[0], lm.recurrence(grid, w_hh, F32)[0]


@pytest.mark.parametrize('frames', [1, 2])
@pytest.mark.parametrize('kernel', sorted(GATE_RUNNERS))
def test_gate_arithmetic(kernel, frames):
    grid, w_hh, truth, want = gate_truth(frames)
    got = GATE_RUNNERS[kernel](grid, w_hh)
    if got is None:
        pytest.skip('this device does not hold the 256 workgroups of the one-launch form at once')
    h = got[0].double()
    for t in range(frames):
        g_t, t_t, w_t = h[:, t], truth[:, t], want[:, t].double()
        big = t_t.abs() >= 1e-30
        rel = ((g_t - t_t).abs() / t_t.abs().clamp_min(1e-300))[big] / lm.ULP
        rel_cpu = ((w_t - t_t).abs() / t_t.abs().clamp_min(1e-300))[big] / lm.ULP
        at = int(rel.argmax())
        cell = torch.nonzero(big.reshape(-1))[at].item()
        gi, gf, gg, go = (float(v.reshape(-1)[cell]) for v in grid[t].chunk(4, dim=1))
        print(f'{kernel} frame {t}: worst relative error {float(rel.max()):.2f} ulp at (i, f, g, o) = ({gi}, {gf}, {gg}, {go}); rms {lm.rms(rel):.2f} ulp; '
              f'the fp32 restatement {float(rel_cpu.max()):.2f} ulp; bound {GATE_BOUND_ULP[t]}')
        for lo, hi in ((-1e9, -50), (-50, -20), (-20, -10), (-10, 1e9)):                   # (information: where the error sits, by the most negative sigmoid argument)
            arg = torch.minimum(grid[t].chunk(4, dim=1)[0], grid[t].chunk(4, dim=1)[3]).double()
            if t:
                arg = torch.minimum(arg, grid[t].chunk(4, dim=1)[1].double())
            sel = ((arg >= lo) & (arg < hi))[big]
            if bool(sel.any()):
                print(f'    most negative sigmoid argument in [{lo}, {hi}): worst {float(rel[sel].max()):.2f} ulp over {int(sel.sum())}')
        small = ~big
        nz = g_t != 0
        assert bool((torch.sign(g_t[nz]) == torch.sign(t_t[nz])).all()), (kernel, t, 'a sign differs from the truth')
        assert bool((g_t[small].abs() < 2e-30).all()), (kernel, t, 'a result below 1e-30 came out above 2e-30')
        assert float(rel.max()) <= GATE_BOUND_ULP[t], (kernel, t, float(rel.max()), (gi, gf, gg, go))


@pytest.mark.parametrize('kernel', sorted(GATE_RUNNERS))
def test_infinite_gates_saturate(kernel):
    """sigmoid(+-Inf) = 1 | 0 and tanh(+-Inf) = +-1 in every kernel: an infinite pre-activation is a saturated gate, not a NaN (the
    compensated exponent of lx_sigmoid computes Inf - Inf on the way and must not let it out).  h stays within 1e-6 of fp64: |h| <= 1
    and a frame is a dozen roundings of 2^-24 each, the bound is sixteen."""
    hidden, batch, frames = 8, 3, 2
    gates, w_hh = (v.clone() for v in reference(hidden, batch, frames)[:2])
    inf = float('inf')
    for t in range(frames):
        for gate, unit, value in ((0, 0, inf), (0, 1, -inf), (1, 2, inf), (1, 3, -inf), (2, 4, inf), (2, 5, -inf), (3, 6, inf), (3, 7, -inf)):
            gates[t, (gate + unit + t) % batch, gate * hidden + unit] = value
    truth = lm.recurrence(gates, w_hh, F64)
    assert bool(torch.isfinite(truth[0]).all()) and bool(torch.isfinite(truth[1]).all())
    got = GATE_RUNNERS[kernel](gates, w_hh)                       # (the runner asserts that h_out and cell_ws are finite)
    assert got is not None
    e_h, e_c = float((got[0].double() - truth[0]).abs().max()), float((got[1].double() - truth[1]).abs().max())
    print(f'{kernel}: infinite gates, worst |h - fp64| {e_h:.2e}, |c - fp64| {e_c:.2e}')
    assert e_h <= 1e-6 and e_c <= 2e-6                             # (|c| <= 2 after two frames)


# ---- E. the exact-fp32 input projection ----------------------------------------------------------------------------------------------------
def proj_cases(axis):
    c0, h0, t0, b0 = lm.PROJ_BASE
    return {'c_in': [(c, h0, t0, b0) for c in lm.PROJ_C_IN], 'hidden': [(c0, h, t0, b0) for h in lm.PROJ_HIDDEN],
            'frames': [(c0, h0, t, b0) for t in lm.PROJ_FRAMES], 'batch': [(c0, h0, t0, b) for b in lm.PROJ_BATCH]}[axis]


def run_projection(xd, frames, w_ih, b_ih, b_hh, hidden, ln):
    batch = xd.shape[0]
    whole, gates = guarded((frames, batch, 4 * hidden))
    hip.lstm_input_projection(xd, frames, w_ih, b_ih, b_hh, gates, hidden, ln)
    torch.cuda.synchronize()
    assert guards_intact(whole), 'lstm_input_projection wrote outside gates_ws'
    out = gates.cpu()
    assert bool(torch.isfinite(out).all()), 'an element of gates_ws was not written'
    return out


def normalised(x, stats, gamma, beta, frames, dtype):
    """The LayerNorm of x (b, c, t) from GIVEN statistics (b, 2, ld), in ``dtype``."""
    x, stats, gamma, beta = (v.to(dtype) for v in (x, stats, gamma, beta))
    return (x - stats[:, 0:1, :frames]) * stats[:, 1:2, :frames] * gamma[None, :, None] + beta[None, :, None]


def batch_first(x):
    """(b, c, t) -> (b, t, c) CONTIGUOUS, as nn.LSTM(batch_first) and the head are handed their input: the operand layout decides which
    routine the CPU's matmul takes, and with it the error that is the yardstick here (a strided operand: rms 1.1e-7 at K = 36 where the
    contiguous one gives 1.6e-7)."""
    return x.permute(0, 2, 1).contiguous()


def projected(x, w_ih, b_ih, b_hh):
    """The first line of oracle.asr_oracle.lstm_forward_loop on x (b, c, t), time-major as the kernel stores it: (t, b, 4H)."""
    return (batch_first(x) @ w_ih.t() + (b_ih + b_hh)).permute(1, 0, 2).contiguous()


def pitched(x, frames):
    b, c, _ = x.shape
    xd = torch.zeros(b, c, hip.row_pitch(frames), device=DEV)
    xd[:, :, :frames] = x.to(DEV)
    return xd


def deferred_ln(xd, frames, gen):
    """(stats on the device from hip.channel_stats, gamma, beta) of x's pending LayerNorm."""
    b, c, ld = xd.shape
    stats = torch.zeros(b, 2, ld, device=DEV)
    hip.channel_stats(xd, stats, frames, EPS)
    return stats, (torch.rand(c, generator=gen) + 0.5).to(DEV), (torch.randn(c, generator=gen) * 0.2).to(DEV)


@functools.lru_cache(maxsize=None)
def projection_reference(c_in, hidden, frames, batch, with_ln):
    """One draw per shape and both CPU products of it, computed once: (x, (w_ih, b_ih, b_hh), ln or None, truth, want); ln = (stats of ALL
    frames from hip.channel_stats, gamma, beta) on the CPU, truth and want (frames, batch, 4H) from those statistics."""
    gen = torch.Generator().manual_seed(c_in * 7919 + hidden * 31 + frames * 3 + batch)
    x = torch.randn(batch, c_in, frames, generator=gen) * 1.5 + 0.3
    w_ih = torch.randn(4 * hidden, c_in, generator=gen) * (1.0 / c_in ** 0.5)
    b_ih, b_hh = torch.randn(4 * hidden, generator=gen) * 0.2, torch.randn(4 * hidden, generator=gen) * 0.2
    ln, x64, x32 = None, x.double(), x
    if with_ln:
        xd = pitched(x, frames)
        stats = torch.zeros(batch, 2, xd.shape[2], device=DEV)
        hip.channel_stats(xd, stats, frames, EPS)
        ln = (stats.cpu(), torch.rand(c_in, generator=gen) + 0.5, torch.randn(c_in, generator=gen) * 0.2)
        x64, x32 = (normalised(x, *ln, frames, dt) for dt in (F64, F32))
    truth, want = (projected(v, w_ih.to(dt), b_ih.to(dt), b_hh.to(dt)) for v, dt in ((x64, F64), (x32, F32)))
    return x, (w_ih, b_ih, b_hh), ln, truth, want


@pytest.mark.parametrize('with_ln', [False, True], ids=['plain', 'ln'])
@pytest.mark.parametrize('axis', ['c_in', 'hidden', 'frames', 'batch'])
def test_input_projection_vs_fp64(axis, with_ln):
    """The frame counts are prefixes of ONE draw of 129 frames and of its reference (a frame's gates depend on that frame alone): the CPU's
    product of a 3-row operand (T = 1, B = 3) is another routine with another error (rms 1.26e-7 where the 129-frame one gives 1.9e-7 on
    those rows), and the yardstick is to be one routine along the axis."""
    fam = lm.Family(f'projection {axis}{" ln" if with_ln else ""}')
    for c_in, hidden, frames, batch in proj_cases(axis):
        x, weights, ln_cpu, truth, want = projection_reference(c_in, hidden, max(lm.PROJ_FRAMES) if axis == 'frames' else frames, batch, with_ln)
        xd, dev = pitched(x[:, :, :frames], frames), [v.to(DEV) for v in weights]
        ln = None
        if with_ln:
            stats = torch.zeros(batch, 2, xd.shape[2])
            stats[:, :, :frames] = ln_cpu[0][:, :, :frames]
            ln = (stats.to(DEV), ln_cpu[1].to(DEV), ln_cpu[2].to(DEV))
        got = run_projection(xd, frames, *dev, hidden, ln)
        fam.add(f'c_in {c_in} H {hidden} T {frames} B {batch}', got, want[:frames], truth[:frames])
        for u in range(batch):
            ln_u = None if ln is None else (ln[0][u:u + 1].contiguous(), ln[1], ln[2])
            alone = run_projection(xd[u:u + 1].contiguous(), frames, *dev, hidden, ln_u)
            assert same_bits(alone[:, 0], got[:, u]), f'utterance {u} alone differs from the batch'
    fam.close()


# ---- F. the head ------------------------------------------------------------------------------------------------------------------------
def head_cases(axis):
    r0, f0, c0 = lm.HEAD_BASE
    return {'rows': [(r, f0, c0) for r in lm.HEAD_ROWS], 'features': [(r0, f, c0) for f in lm.HEAD_FEATURES],
            'classes': [(r0, f0, c) for c in lm.HEAD_CLASSES]}[axis]


def head_weights(features, classes, gen):
    return torch.randn(classes, features, generator=gen) * 0.05, torch.randn(classes, generator=gen)


@functools.lru_cache(maxsize=None)
def head_reference(rows, features):
    """One draw per (rows, features) with all 64 classes, and both CPU products of it, computed once: a case of fewer classes takes the
    first of them.  (So the yardstick is one routine whatever the class count: for ONE class the CPU's product is a matrix-vector
    routine with another summation, rms 3.6e-8 where every other count gives 7.2e-8 at 132 features.)"""
    gen = torch.Generator().manual_seed(rows * 7919 + features * 31)
    h = torch.rand(rows, features, generator=gen) * 2 - 1                                  # an LSTM's output: |h| <= 1
    w, b = head_weights(features, 64, gen)
    return h, w, b, h.double() @ w.double().t() + b.double(), h @ w.t() + b


@pytest.mark.parametrize('axis', ['rows', 'features', 'classes'])
def test_linear_head_vs_fp64(axis):
    fam = lm.Family(f'head {axis}')
    for rows, features, classes in head_cases(axis):
        h, w, b, truth, want = head_reference(rows, features)
        whole, logits = guarded((rows, classes))
        hip.linear_head(h.to(DEV), w[:classes].contiguous().to(DEV), b[:classes].contiguous().to(DEV), logits)
        torch.cuda.synchronize()
        assert guards_intact(whole), 'linear_head wrote outside logits'
        fam.add(f'rows {rows} features {features} classes {classes}', logits.cpu(), want[:, :classes], truth[:, :classes])
    fam.close()


@pytest.mark.parametrize('with_ln', [False, True], ids=['plain', 'ln'])
def test_linear_head_bct_vs_fp64(with_ln):
    fam = lm.Family(f'head bct{" ln" if with_ln else ""}')
    _, _, classes = lm.HEAD_BASE
    for (batch, frames), features in [(bt, f) for bt in lm.HEAD_BCT for f in (36, 132)]:
        gen = torch.Generator().manual_seed(batch * 7919 + frames * 31 + features)
        x = torch.randn(batch, features, frames, generator=gen) * 1.5 + 0.3
        w, b = head_weights(features, classes, gen)
        xd = pitched(x, frames)
        assert xd.shape[2] > frames                                                        # there ARE pitch columns
        ln = deferred_ln(xd, frames, gen) if with_ln else None
        whole, logits = guarded((batch, frames, classes))
        hip.linear_head_bct(xd, frames, w.to(DEV), b.to(DEV), logits, ln)
        torch.cuda.synchronize()
        assert guards_intact(whole), 'linear_head_bct wrote outside logits'
        if with_ln:
            stats, gamma, beta = (v.cpu() for v in ln)
            x64, x32 = (normalised(x, stats, gamma, beta, frames, dt) for dt in (F64, F32))
        else:
            x64, x32 = x.double(), x
        fam.add(f'B {batch} T {frames} features {features}', logits.cpu(), batch_first(x32) @ w.t() + b, batch_first(x64) @ w.double().t() + b.double())
    fam.close()


def test_linear_head_refuses_65_classes():
    h, w, b = torch.zeros(4, 8, device=DEV), torch.zeros(65, 8, device=DEV), torch.zeros(65, device=DEV)
    with pytest.raises(hip.HipError):
        hip.linear_head(h, w, b, torch.zeros(4, 65, device=DEV))
    with pytest.raises(hip.HipError):
        hip.linear_head_bct(torch.zeros(1, 8, 4, device=DEV), 4, w, b, torch.zeros(1, 4, 65, device=DEV))
