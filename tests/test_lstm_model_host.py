"""tests/lstm_model.py against torch's own LSTM, its carried state, and what its fp32 form can deliver; no GPU.

The restatement is the yardstick of tests/test_recurrent_edges_gpu.py, so it is itself held to an independent evaluation (torch._VF.lstm
in fp64, to 1e-12), and its fp32 form's distance to fp64 -- the e_ref every kernel there is measured in -- is printed at the edge shapes
(measured: H = 520, B = 17, T = 9, w ~ 0.2: rms 1.4e-7, worst 2.1e-6; H = 4, B = 3, T = 5: rms 1.2e-8, worst 2.9e-8; the cell state
roughly 3 x those)."""
import pytest
import torch

import lstm_model as lm

F32, F64 = torch.float32, torch.float64


@pytest.mark.parametrize('hidden', [4, 36])
def test_recurrence_is_torch_lstm_in_fp64(hidden):
    b, t = 3, 5
    gen = torch.Generator().manual_seed(hidden)
    x = torch.randn(b, t, 7, generator=gen, dtype=F64)
    w_ih, w_hh = torch.randn(4 * hidden, 7, generator=gen, dtype=F64) * 0.4, torch.randn(4 * hidden, hidden, generator=gen, dtype=F64) * 0.3
    b_ih, b_hh = torch.randn(4 * hidden, generator=gen, dtype=F64) * 0.2, torch.randn(4 * hidden, generator=gen, dtype=F64) * 0.2
    h0, c0 = torch.randn(b, hidden, generator=gen, dtype=F64) * 0.5, torch.randn(b, hidden, generator=gen, dtype=F64)
    gates = (x @ w_ih.t() + (b_ih + b_hh)).permute(1, 0, 2).contiguous()
    for state in (None, (h0, c0)):
        hx = (torch.zeros(1, b, hidden, dtype=F64),) * 2 if state is None else (h0[None], c0[None])
        want, _, c_want = torch._VF.lstm(x, hx, [w_ih, w_hh, b_ih, b_hh], True, 1, 0.0, False, False, True)
        got, c_got = lm.recurrence(gates, w_hh, F64, *(state or (None, None)))
        assert got.dtype == F64 and got.shape == (b, t, hidden) and c_got.shape == (b, hidden)
        assert float((got - want).abs().max()) <= 1e-12 and float((c_got - c_want[0]).abs().max()) <= 1e-12


@pytest.mark.parametrize('dtype', [F32, F64])
def test_a_run_split_at_a_frame_boundary_is_the_unsplit_run(dtype):
    gates, w_hh = lm.draw(36, 3, 5)
    whole, c_whole = lm.recurrence(gates, w_hh, dtype)
    for cut in range(1, 5):
        head, c_head = lm.recurrence(gates[:cut], w_hh, dtype)
        tail, c_tail = lm.recurrence(gates[cut:], w_hh, dtype, h0=head[:, -1], c0=c_head)
        assert torch.equal(torch.cat([head, tail], dim=1), whole) and torch.equal(c_tail, c_whole), cut


def test_gates_fn_is_one_frame_of_the_recurrence():
    gates, w_hh = lm.draw(8, 3, 1)
    i, f, g, o = gates[0].chunk(4, dim=1)
    c, h = lm.gates_fn(i, f, g, o, torch.zeros(3, 8), F64)
    want, c_want = lm.recurrence(gates, w_hh, F64)
    assert torch.equal(h, want[:, 0]) and torch.equal(c, c_want) and h.dtype == F64


def test_the_gate_grid_holds_every_value_in_every_role():
    grid = lm.gate_grid(2)
    b, hid = lm.GATE_GRID
    assert grid.shape == (2, b, 4 * hid) and torch.equal(grid[0], grid[1])
    values = sorted(set(lm.GATE_VALUES))                             # (+0 and -0 compare equal: 104 distinct numbers)
    for role in grid[0].chunk(4, dim=1):
        assert sorted(set(role.reshape(-1).tolist())) == sorted(set(torch.tensor(values).tolist()))
        assert bool((role == 0).any()) and bool(torch.signbit(role[role == 0]).any()) and not bool(torch.signbit(role[role == 0]).all())
    # the fp32 evaluation of the whole grid is finite and close to fp64 wherever the result is a normal number
    for frames in (1, 2):
        truth, _ = lm.recurrence(lm.gate_grid(frames), torch.zeros(4 * hid, hid), F64)
        want, _ = lm.recurrence(lm.gate_grid(frames), torch.zeros(4 * hid, hid), F32)
        assert bool(torch.isfinite(want).all())
        big = truth.abs() >= 1e-30
        rel = float(((want.double() - truth).abs()[big] / truth.abs()[big]).max())
        print(f'gate grid, {frames} frame(s): fp32 restatement within {rel:.2e} relative of fp64 over {int(big.sum())} results')
        assert rel <= 9 * lm.ULP


@pytest.mark.parametrize('hidden,batch,frames,scale', [(520, 17, 9, 0.2), (4, 3, 5, 0.3), (36, 17, 3, 0.3), (1024, 17, 3, 0.1), (500, 33, 3, 0.1)])
def test_print_what_the_fp32_restatement_delivers(hidden, batch, frames, scale):
    gen = torch.Generator().manual_seed(hidden + batch)
    gates, w_hh = torch.randn(frames, batch, 4 * hidden, generator=gen), torch.randn(4 * hidden, hidden, generator=gen) * scale
    truth, c_truth = lm.recurrence(gates, w_hh, F64)
    want, c_want = lm.recurrence(gates, w_hh, F32)
    e_h, e_c = (want.double() - truth).abs(), (c_want.double() - c_truth).abs()
    print(f'H {hidden} B {batch} T {frames} w ~ {scale}: h rms {lm.rms(e_h):.2e} worst {float(e_h.max()):.2e} | c_T rms {lm.rms(e_c):.2e} worst {float(e_c.max()):.2e}')
    assert want.dtype == F32 and 0 < lm.rms(e_h) < 1e-6 and float(e_h.max()) < 2e-5 and lm.rms(e_c) < 3e-6     # fp32 round-off, not a bug's size
