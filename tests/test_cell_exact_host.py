"""The exactly summable cell operands of ``tests/cell_exact.py``, checked without a GPU: for every case the GPU file runs, the conditions
that make an element-by-element equality meaningful (integers within bf16's exact range, enough pre-activations that relu and the clamp
let through, every (input channel, tap) weighted), and hand-computed answers of the fp64 reference."""
import pytest
import torch

import cell_exact as ce
from oracle import asr_oracle as oracle


def _id(case):
    return f'cg{case.cg}-g{case.groups}-t{case.t}-m{case.mask}-' + ''.join(f'{k}{d}' for k, d in case.kds)


@pytest.mark.parametrize('case', ce.all_cases(), ids=_id)
def test_conditions_hold_for_every_gpu_case(case):
    """(a) integer-valued tensors and partial sums of magnitude <= 256, (b) >= 0.2 of every node's pre-activations strictly inside
    (0, 20), (c) every (input channel, tap) of every node weighted in some group.  Over the cases: shares 0.26 .. 0.9, magnitudes <= 106."""
    shares = ce.check_conditions(case)
    ops, ref = ce.operands(case), ce.reference(case)
    assert ref.x3.shape == (case.batch, case.cg * case.groups, case.t)
    for i, (w, bias, _, d) in enumerate(ops.nodes):                      # the pre-activations belong to the activations the chain used
        src = (ref.x0n, ref.x1, ref.x2)[i]
        assert torch.equal(torch.clamp(torch.relu(ref.pre[i]), max=oracle.CLAMP), oracle.pad_conv_relu(src, w, bias, d, 1, case.groups))
    assert all(0.0 < s <= 1.0 for s in shares)


def test_the_gpu_cases_cover_what_they_promise():
    forced = ce.mfma_forced_cases()
    for cg in ce.CGS:
        assert {nbt for c, nbt, _ in forced if c == cg} == set(ce.mfma_nbts(cg))
    assert ce.mfma_frames(16) == (1, 7, 8, 9, 127, 129, 255, 256, 257, 271, 513)
    assert ce.mfma_frames(10) == (1, 7, 8, 9, 79, 81, 159, 160, 161, 175, 321)
    assert max(c.t * c.cg * c.groups for c in ce.all_cases()) == 513 * 48          # the largest case: 48 channels x 513 frames x 2 utterances
    masks = {c.mask for c in ce.all_cases()}
    assert {0, 63, 0b101001, 0b010110} <= masks
    assert {c.groups for c in ce.mfma_other_cases()} == {4, 5, 6}
    # operands are keyed: the same case gives the same tensors, another case others
    a, b = ce.case(6, 9, ce.COMBO_LN), ce.case(6, 9, ce.COMBO_PLAIN)
    ce.operands.cache_clear()
    first = ce.operands(a).x0.clone()
    ce.operands.cache_clear()
    assert torch.equal(ce.operands(a).x0, first) and not torch.equal(ce.operands(b).x0, first)


@pytest.mark.parametrize('k,d', [(5, 1), (5, 2), (7, 1), (7, 2)])
def test_a_one_hot_weight_moves_an_impulse_by_tap_times_dilation_minus_the_left_padding(k, d):
    """y[f] = sum_tap w[tap] x[f + tap d - left]: one weight at `tap` carries an impulse at frame f0 to frame f0 - (tap d - left).  The
    left paddings written out by hand from the reference's look-ahead rule (4 frames of look-ahead at stride 1)."""
    left = {(5, 1): 0, (5, 2): 4, (7, 1): 2, (7, 2): 8}[(k, d)]
    assert oracle.pad_amounts(k, d, 1) == (left, 4)
    t, f0, cg, groups = 40, 20, 6, 2
    for tap in range(k):
        x = torch.zeros(1, cg * groups, t, dtype=torch.float64)
        x[0, cg + 3, f0] = 5.0                                           # input channel 3 of group 1
        w = torch.zeros(cg * groups, cg, k, dtype=torch.float64)
        w[cg + 1, 3, tap] = 1.0                                          # -> output channel 1 of group 1
        w[2, 3, tap] = 1.0                                               # (group 0 sees no impulse)
        bias = torch.zeros(cg * groups, dtype=torch.float64)
        ops = ce.Operands(x, None, ((w, bias, k, d),) * 3)
        ref = ce.evaluate(ops, ce.Case(cg, groups, t, ((k, d),) * 3, 0, False, 1))
        want = torch.zeros_like(x)
        want[0, cg + 1, f0 - (tap * d - left)] = 5.0
        assert torch.equal(ref.x1, want) and torch.equal(ref.pre[0], want), tap


def test_a_hand_computed_cell_with_layernorm_clamp_and_skips():
    """One group of 6 channels, 3 frames, conv5 (no left padding, 4 frames of look-ahead) in every node, every skip on:
        x0 = 2 in channel 0, frames 0..2, mean 1, rstd 2, gamma -1 / beta 1 in channel 0:   x0n[0] = (2 - 1) 2 (-1) + 1 = -1, the other
        channels (x0 = 0, gamma 1, beta 0): (0 - 1) 2 = -2.
      node 0: w[co 0] = -1 on (channel 0, taps 0 and 1), bias 3: pre = 3 + 1 + 1 = 5 at frames 0, 1 (both taps inside the row), 3 + 1 = 4 at
        frame 2 (tap 1 reads the padding); x1[0] = pre + x0n[0] = 4, 4, 3.  The other output channels: bias 0, relu(0) + x0n = -2.
      node 1: w[co 0] = 6 on (channel 0, tap 0): pre = 24, 24, 18 -> clamp 20, 20, 18; x2[0] = . + x0n[0] + x1[0] = 23, 23, 20.
      node 2: w[co 0] = -1 on (channel 0, tap 0): pre = -23 .. -> 0; x3[0] = x0n + x1 + x2 = 26, 26, 22; the others -2 -2 -4 = -8."""
    cg, t = 6, 3
    x0 = torch.zeros(1, cg, t, dtype=torch.float64)
    x0[0, 0] = 2.0
    gamma, beta = torch.ones(cg, dtype=torch.float64), torch.zeros(cg, dtype=torch.float64)
    gamma[0], beta[0] = -1.0, 1.0
    ln = (torch.ones(1, t, dtype=torch.float64), torch.full((1, t), 2.0, dtype=torch.float64), gamma, beta)
    ws = [torch.zeros(cg, cg, 5, dtype=torch.float64) for _ in range(3)]
    ws[0][0, 0, 0] = ws[0][0, 0, 1] = -1.0
    ws[1][0, 0, 0] = 6.0
    ws[2][0, 0, 0] = -1.0
    b0 = torch.zeros(cg, dtype=torch.float64)
    b0[0] = 3.0
    zero = torch.zeros(cg, dtype=torch.float64)
    ops = ce.Operands(x0, ln, ((ws[0], b0, 5, 1), (ws[1], zero, 5, 1), (ws[2], zero, 5, 1)))
    ref = ce.evaluate(ops, ce.Case(cg, 1, t, ((5, 1),) * 3, 63, True, 1))
    assert ref.x0n[0, 0].tolist() == [-1.0, -1.0, -1.0] and ref.x0n[0, 1].tolist() == [-2.0, -2.0, -2.0]
    assert ref.pre[0][0, 0].tolist() == [5.0, 5.0, 4.0] and ref.x1[0, 0].tolist() == [4.0, 4.0, 3.0]
    assert ref.pre[1][0, 0].tolist() == [24.0, 24.0, 18.0] and ref.x2[0, 0].tolist() == [23.0, 23.0, 20.0]
    assert ref.x3[0, 0].tolist() == [26.0, 26.0, 22.0]
    assert ref.x1[0, 1].tolist() == [-2.0] * 3 and ref.x2[0, 1].tolist() == [-4.0] * 3 and ref.x3[0, 1].tolist() == [-8.0] * 3


def test_moving_one_tap_changes_the_reference():
    """The premise of the GPU file's sensitivity test: one weight of the last node on the neighbouring tap is another x3."""
    ops = ce.operands(ce.SENSITIVITY)
    moved, (co, ci, tap, new) = ce.move_one_tap(ops)
    w, w2 = ops.nodes[2][0], moved.nodes[2][0]
    assert abs(new - tap) == 1 and int((w != w2).sum()) == 2 and w2[co, ci, new] == w[co, ci, tap] != 0 and w2[co, ci, tap] == 0
    assert all(torch.equal(a[0], b[0]) for a, b in zip(ops.nodes[:2], moved.nodes[:2]))
    got, want = ce.evaluate(moved, ce.SENSITIVITY), ce.reference(ce.SENSITIVITY)
    assert torch.equal(got.x2, want.x2)
    differs = (got.x3 != want.x3)
    assert bool(differs.any()) and bool(differs[:, co].any()) and not bool(differs[:, :co].any()) and not bool(differs[:, co + 1:].any())
