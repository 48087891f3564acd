"""``nbasr_dropout`` on the device against its numpy definition (tests/dropout_model.py), bit for bit: operator shapes, the loop edges
of the kernel (grid limit, partial last group, 64-bit group numbers, sign extension, aliasing), the fused node sum against dropout
followed by the skip-sum launches, autograd, and the model's training path with ``dropout.use('hip')``."""
import numpy as np
import pytest
import torch

import cases
import dropout_model as dm
import nb_asr_amd as nb
from nb_asr_amd import autograd as nb_autograd, dropout, hip
from nb_asr_amd.weights import keyed_fill_, keyed_input

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SEED = 20240229                  # tests/test_dropout_host.py checks the model's kept share with it
SITES = 18 * 3 + 1               # dropout sites of a forward of ARCH_D: three node ops in each of the 18 cells, one in front of the LSTM
POISON = 0x7fc0dead              # a NaN payload no arithmetic produces: what the pitch columns hold before a launch


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def values(rows, frames, key=0):
    """Exactly representable, mixed signs, a few zeros of either sign."""
    rng = np.random.default_rng(1000 * rows + frames + key)
    x = (rng.integers(-2000, 2000, size=(rows, frames)) / 64.0).astype(np.float32)
    x[rng.random((rows, frames)) < 0.02] = -0.0
    return x


def on_device(x, ld):
    """(rows, frames) -> a (rows, ld) device tensor, the pitch columns poisoned."""
    buf = np.full((x.shape[0], ld), POISON, dtype=np.uint32)
    buf[:, :x.shape[1]] = bits(x)
    return torch.from_numpy(buf.view(np.float32)).to(DEV)


def run(x, ld, p, seed, call, row0=0, skips=(), inplace=False):
    """One launch; returns the (rows, frames) result after checking that the pitch columns of y are what they were and x is unchanged."""
    rows, frames = x.shape
    xd = on_device(x, ld)
    yd = xd if inplace else on_device(np.zeros_like(x), ld)
    sd = [on_device(s, ld) for s in skips]
    hip.dropout(xd, yd, frames, p, seed, call, sd, row0)
    y = bits(yd.cpu().numpy())
    assert (y[:, frames:] == POISON).all(), 'pitch columns of y were written'
    if not inplace:
        assert np.array_equal(bits(xd.cpu().numpy())[:, :frames], bits(x)), 'x was written'
    for s, d in zip(skips, sd):
        assert np.array_equal(bits(d.cpu().numpy())[:, :frames], bits(s)), 'a skip was written'
    return y[:, :frames]


@pytest.mark.parametrize('frames', [1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1021])
def test_operator_shapes(frames):
    for rows in (1, 3, 257):
        x = values(rows, frames)
        for call, p in enumerate((0, 0.2, 0.5, 1)):
            want = bits(dm.apply(x, p, SEED, call))
            for ld in (hip.round_up4(frames), hip.round_up4(frames) + 8):
                for inplace in (False, True):
                    got = run(x, ld, p, SEED, call, inplace=inplace)
                    assert np.array_equal(got, want), (rows, frames, ld, p, inplace, int((got != want).sum()))
            if p == 0:
                assert np.array_equal(want, bits(x))
            if p == 1:
                assert not (want & 0x7fffffff).any()


def test_rows_beyond_a_grid_dimension():
    x = values(65537, 4)
    assert np.array_equal(run(x, 4, 0.2, SEED, 3), bits(dm.apply(x, 0.2, SEED, 3)))


def test_more_groups_than_the_grid_holds_threads():
    """8192 blocks of 256 threads is the grid's cap: 2 097 152 groups per sweep; 2100 rows of 1001 groups need a second one, and the
    stride is no multiple of a row."""
    x = values(2100, 4001)
    want = bits(dm.apply(x, 0.5, SEED, 4))
    assert np.array_equal(run(x, 4004, 0.5, SEED, 4), want) and np.array_equal(run(x, 4012, 0.5, SEED, 4, inplace=True), want)


def test_group_number_crosses_2_32():
    x = values(2, 8)
    row0 = (1 << 31) - 1
    want = dm.apply(x, 0.5, SEED, 0, row0)
    assert np.array_equal(run(x, 8, 0.5, SEED, 0, row0), bits(want))
    assert not np.array_equal(bits(want), bits(dm.apply(x, 0.5, SEED, 0, row0 - (1 << 31))))        # the high word of g counts


def test_seed_and_call_are_64_bit_patterns():
    x = values(5, 37)
    got = run(x, 40, 0.5, -1, -(1 << 63))
    assert np.array_equal(got, bits(dm.apply(x, 0.5, (1 << 64) - 1, 1 << 63)))
    for seed, call in (((1 << 32) - 1, 1 << 63), (-1, 0), ((1 << 63) - 1, -(1 << 63))):             # no half is dropped or smeared
        other = run(x, 40, 0.5, seed, call)
        assert np.array_equal(other, bits(dm.apply(x, 0.5, seed, call))) and not np.array_equal(other, got)


def test_row_slices_equal_the_whole():
    x = values(23, 45)
    whole = run(x, 48, 0.2, SEED, 7)
    parts = [run(x[a:b], 48, 0.2, SEED, 7, row0=a) for a, b in ((0, 5), (5, 6), (6, 23))]
    assert np.array_equal(np.concatenate(parts), whole) and np.array_equal(whole, bits(dm.apply(x, 0.2, SEED, 7)))


def test_determinism():
    x = values(9, 130)
    a, b, c = run(x, 132, 0.2, SEED, 8), run(x, 132, 0.2, SEED, 8), run(x, 132, 0.2, SEED, 9)
    assert np.array_equal(a, b) and not np.array_equal(a, c)


def test_non_finite_values():
    x = values(6, 50)
    x[:, 0::5], x[:, 1::5], x[:, 2::5] = np.inf, -np.inf, np.nan
    want = dm.apply(x, 0.5, SEED, 10)
    m = dm.multiplier(6, 50, 0.5, SEED, 10)
    assert np.isnan(want[:, 0::5][m[:, 0::5] == 0]).all() and np.isinf(want[:, 0::5][m[:, 0::5] != 0]).all()       # both places occur
    assert (m[:, 0::5] == 0).any() and (m[:, 0::5] != 0).any()
    got = run(x, 52, 0.5, SEED, 10)
    finite = ~np.isnan(want)
    assert np.array_equal(np.isnan(got.view(np.float32)), ~finite) and np.array_equal(got[finite], bits(want)[finite])


@pytest.mark.parametrize('n', [1, 2, 3])
def test_fused_node_sum(n):
    """Equal to hip.dropout followed by hip.skip_sum as autograd._SkipSum strings them, and to the model."""
    b, c, frames = 2, 7, 61
    ld = hip.round_up4(frames)
    x = values(b * c, frames)
    skips = [values(b * c, frames, key=k + 1) for k in range(n)]
    want = bits(dm.apply(x, 0.2, SEED, 11, skips=skips))
    for inplace in (False, True):
        assert np.array_equal(run(x, ld, 0.2, SEED, 11, skips=skips, inplace=inplace), want), inplace

    def pitched(a):
        t = torch.zeros(b, c, ld, device=DEV)
        t[:, :, :frames] = torch.from_numpy(a).reshape(b, c, frames).to(DEV)
        return t
    dropped = hip.dropout(pitched(x), torch.zeros(b, c, ld, device=DEV), frames, 0.2, SEED, 11)
    apart = nb_autograd._SkipSum.apply(dropped[:, :, :frames], *[pitched(s)[:, :, :frames] for s in skips])
    assert np.array_equal(bits(apart.cpu().numpy()).reshape(b * c, frames), want)


def test_autograd():
    b, c, frames = 2, 5, 10                                     # 10 frames: pitched to 12 on the way in and out
    x = torch.from_numpy(values(b * c, frames)).reshape(b, c, frames).to(DEV).requires_grad_(True)
    skips = [torch.from_numpy(values(b * c, frames, key=k + 1)).reshape(b, c, frames).to(DEV).requires_grad_(True) for k in range(2)]
    dy = torch.from_numpy(values(b * c, frames, key=9)).reshape(b, c, frames).to(DEV)
    saved = dropout.get_state()
    try:
        dropout.manual_seed(SEED)
        dropout.dropout(x, 0.2)                                 # call 0
        y = dropout.dropout(x, 0.2, True, skips)                # call 1
        assert dropout.get_state() == (SEED, 2) and y.grad_fn.saved_tensors == ()
        flat = lambda t: t.detach().cpu().numpy().reshape(b * c, frames)
        assert np.array_equal(bits(flat(y)), bits(dm.apply(flat(x), 0.2, SEED, 1, skips=[flat(s) for s in skips])))
        y.backward(dy)
        assert np.array_equal(bits(flat(x.grad)), bits(dm.apply(flat(dy), 0.2, SEED, 1)))          # mask * scale * dy
        assert all(np.array_equal(bits(flat(s.grad)), bits(flat(dy))) for s in skips)
        assert dropout.get_state() == (SEED, 2)                 # backward takes no call
    finally:
        dropout.set_state(saved)


def test_slices_of_pitched_buffers_are_taken_without_a_copy():
    """What the ops return when the frame count is no multiple of 4: x, the skip and the gradient are read where they lie (no re-pitch
    launch), nothing of theirs is written, pitch columns included; a slice that does not start a 16-byte group is copied."""
    b, c, frames, ld = 2, 5, 10, 12
    host = {k: values(b * c, frames, key=k) for k in range(3)}
    buf = {k: on_device(v, ld).reshape(b, c, ld) for k, v in host.items()}
    before = {k: v.clone() for k, v in buf.items()}
    whole = torch.from_numpy(values(b * c, ld, key=3)).reshape(b, c, ld).to(DEV)
    x = buf[0][:, :, :frames].requires_grad_(True)
    skip = buf[1][:, :, :frames].requires_grad_(True)
    saved = dropout.get_state()
    entries = []
    hip.start_tape(entries)
    try:
        dropout.manual_seed(SEED)
        y = dropout.dropout(x, 0.5, True, [skip])
        y.backward(buf[2][:, :, :frames])
        shifted = dropout.dropout(whole[:, :, 1:11], 0.5)                     # call 1: the same strides, but off the 16-byte groups
    finally:
        hip.stop_tape()
        dropout.set_state(saved)
    # (the tape follows this thread: the forward launches; backward runs on autograd's own)
    assert [fn.__name__ for fn, _ in entries] == ['nbasr_dropout', 'nbasr_repitch', 'nbasr_dropout']
    flat = lambda t: t.detach().cpu().numpy().reshape(b * c, -1)
    assert np.array_equal(bits(flat(y)), bits(dm.apply(host[0], 0.5, SEED, 0, skips=[host[1]])))
    assert np.array_equal(bits(flat(x.grad)), bits(dm.apply(host[2], 0.5, SEED, 0)))
    assert np.array_equal(bits(flat(skip.grad)), bits(host[2]))
    assert np.array_equal(bits(flat(shifted)), bits(dm.apply(flat(whole)[:, 1:11], 0.5, SEED, 1)))
    assert all(np.array_equal(bits(flat(buf[k])), bits(flat(before[k]))) for k in buf)


@pytest.fixture
def hip_backend():
    saved = dropout.get_state()
    with dropout.use('hip'):
        yield
    dropout.set_state(saved)


@pytest.fixture(scope='module')
def model():
    m = nb.get_model(cases.ARCH_D, use_rnn=True, dropout_rate=0.2)
    keyed_fill_(m, 5, 'lively')
    return m.to(DEV), keyed_input(2, 40, seed=2).to(DEV)


def grads(m):
    return [p.grad.clone() for p in m.parameters()]


def test_model_training_path(hip_backend, model, monkeypatch):
    m, x = model
    m.train()

    def refuse(*args, **kwargs):
        raise AssertionError("ATen's dropout was reached with the hip backend")
    monkeypatch.setattr(torch.nn.functional, 'dropout', refuse)
    dropout.manual_seed(SEED)
    a, b = m(x), m(x)
    assert a.grad_fn is not None and not torch.equal(a, b)
    sites = dropout.get_state()[1] // 2
    assert sites == SITES
    m.zero_grad()
    a.sum().backward()
    first = grads(m)
    assert all(bool(torch.isfinite(g).all()) for g in first) and dropout.get_state() == (SEED, 2 * sites)
    # replay from the seed: logits and every gradient, to the bit
    dropout.manual_seed(SEED)
    a2 = m(x)
    m.zero_grad()
    a2.sum().backward()
    assert torch.equal(a2, a) and all(torch.equal(g, h) for g, h in zip(grads(m), first))
    # the forward without gradients draws the same masks
    dropout.manual_seed(SEED)
    with torch.no_grad():
        c = m(x)
    assert c.grad_fn is None and torch.equal(c, a) and dropout.get_state() == (SEED, sites)
    # a checkpointed state replays the second forward
    state = dropout.get_state()
    with torch.no_grad():
        d = m(x)
        dropout.set_state(state)
        e = m(x)
    assert torch.equal(d, b) and torch.equal(e, d)
    # the executor-only entry points hold no masks in either backend
    with torch.no_grad(), pytest.raises(NotImplementedError, match='dropout'):
        m.forward_async(x)
    with torch.no_grad(), pytest.raises(NotImplementedError, match='dropout'):
        m.forward_graph(x)


def test_one_op_is_its_eval_output_times_the_mask(hip_backend, model):
    m, _ = model
    xin = torch.randn(2, 600, 50, device=DEV)
    for op in (m.model[2].nodes[0].op, m.model[3].nodes[2].op):
        with torch.no_grad():
            seed, call = dropout.get_state()
            y_train = op.train()(xin)
            y_eval = op.eval()(xin)
        assert dropout.get_state() == (seed, call + 1)
        want = dm.apply(y_eval.cpu().numpy().reshape(2 * 600, 50), 0.2, seed, call)
        assert np.array_equal(bits(y_train.cpu().numpy().reshape(2 * 600, 50)), bits(want))
        share = float((want != 0).sum()) / float((y_eval != 0).sum())
        assert abs(share - 0.8) < 0.02, share
    m.train()


def test_eval_and_p_zero_launch_nothing(hip_backend, model):
    m, x = model
    entries = []
    state = dropout.get_state()
    m.eval()
    hip.start_tape(entries)
    try:
        with torch.no_grad():
            m(x)
        m0 = keyed_fill_(nb.get_model(cases.ARCH_D, use_rnn=True, dropout_rate=0.0), 5, 'lively').to(DEV).train()
        m0(x).sum().backward()
    finally:
        hip.stop_tape()
        m.train()
    assert entries and not [fn for fn, _ in entries if fn.__name__ == 'nbasr_dropout'] and dropout.get_state() == state


def test_aten_backend_never_calls_the_entry_point(model):
    m, x = model
    m.train()
    assert dropout.backend() == 'aten'
    entries = []
    state = dropout.get_state()
    hip.start_tape(entries)
    try:
        m(x).sum().backward()
        with torch.no_grad():
            m(x)
    finally:
        hip.stop_tape()
    assert entries and not [fn for fn, _ in entries if fn.__name__ == 'nbasr_dropout'] and dropout.get_state() == state
    # and the hip backend does: one launch per site
    with dropout.use('hip'):
        del entries[:]
        hip.start_tape(entries)
        try:
            with torch.no_grad():
                m(x)
        finally:
            hip.stop_tape()
        dropout.set_state(state)
    launches = [args for fn, args in entries if fn.__name__ == 'nbasr_dropout']
    assert len(launches) == SITES and [a[10] for a in launches] == list(range(state[1], state[1] + SITES))
    assert [sum(s is not None for s in a[1:4]) for a in launches] == [1, 2, 3] * 18 + [0]  # ARCH_D's flagged skips ride in the launch
    assert not [fn for fn, _ in entries if fn.__name__ == 'nbasr_skip_sum']
