"""Counter-based dropout without a GPU: the numpy definition (tests/dropout_model.py) against known answers and its own invariants, the
host-side refusals of ``nbasr_dropout`` through the loaded library, and the state logic of ``nb_asr_amd.dropout`` against a stub library."""
import numpy as np
import pytest
import torch

import dropout_model as dm
import nb_asr_amd as nb
from nb_asr_amd import dropout, hip

SEED = 20240229                  # the seed tests/test_dropout_gpu.py uses

KNOWN = [      # (counter x 4, key x 2) -> output x 4: the Random123 known-answer vectors of philox4x32_10
    ([0, 0, 0, 0], [0, 0], [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]),
    ([0xffffffff] * 4, [0xffffffff] * 2, [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]),
    ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0], [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]),
]


def test_generator_known_answers():
    for counter, key, want in KNOWN:
        assert dm.philox4x32_10(np.array(counter, dtype=np.uint32), key).tolist() == want
    batch = dm.philox4x32_10(np.array([k[0] for k in KNOWN[:1]] * 3, dtype=np.uint32), KNOWN[0][1])       # vectorised over counters
    assert batch.tolist() == [KNOWN[0][2]] * 3


def test_threshold_and_scale():
    assert dm.thr(0) == 0 and dm.scale(0) == np.float32(1)
    assert dm.thr(0.2) == 858993459 and dm.scale(0.2) == np.float32(1.25)
    assert dm.thr(0.5) == 1 << 31 and dm.scale(0.5) == np.float32(2)
    assert dm.thr(1 - 2.0 ** -33) == 1 << 32 and dm.scale(1 - 2.0 ** -33) == np.float32(2.0 ** 33)
    assert dm.thr(1) == 1 << 32 and dm.scale(1) == np.float32(0)
    assert dm.kept(3, 9, 0, SEED, 0).all() and not dm.kept(3, 9, 1, SEED, 0).any() and not dm.kept(3, 9, 1 - 2.0 ** -33, SEED, 0).any()
    x = np.arange(27, dtype=np.float32).reshape(3, 9) - 5
    assert np.array_equal(dm.apply(x, 0, SEED, 0), x) and not dm.apply(x, 1, SEED, 0).any()
    for bad in (-1e-9, 1.0000001, float('nan')):
        with pytest.raises(ValueError):
            dm.thr(bad)


def test_kept_share():
    """2^20 Bernoulli(0.8) draws: the share's standard deviation is sqrt(0.16 / 2^20) = 3.9e-4; five of them."""
    share = dm.kept(1024, 1024, 0.2, SEED, 0).mean()
    assert abs(share - 0.8) < 2e-3, share


def test_mask_is_a_function_of_seed_call_row_and_frame():
    rows, frames = 7, 13
    w = dm.words(rows, frames, SEED, 5)
    # groups never straddle rows: row r, frame t takes word t & 3 of group r * 4 + t // 4
    gpr = dm.groups_per_row(frames)
    assert gpr == 4
    for r, t in ((0, 0), (2, 5), (6, 12)):
        g = r * gpr + t // 4
        assert w[r, t] == dm.philox4x32_10(np.array([g, 0, 5, 0], dtype=np.uint32), [SEED & dm.MASK32, SEED >> 32])[t & 3]
    # slices with row0 equal the whole
    assert np.array_equal(np.concatenate([dm.words(2, frames, SEED, 5, 0), dm.words(4, frames, SEED, 5, 2), dm.words(1, frames, SEED, 5, 6)]), w)
    # another call or another seed is another mask; the high halves count
    for seed, call in ((SEED, 6), (SEED + 1, 5), (SEED, 5 + (1 << 32)), (SEED + (1 << 32), 5)):
        assert (dm.words(rows, frames, seed, call) != w).mean() > 0.9
    # negative seed / call are their unsigned patterns
    assert np.array_equal(dm.words(rows, frames, -1, -(1 << 63)), dm.words(rows, frames, (1 << 64) - 1, 1 << 63))
    assert not np.array_equal(dm.words(rows, frames, -1, -(1 << 63)), dm.words(rows, frames, (1 << 32) - 1, 0))
    # g is a 64-bit number: row0 = 2^31 - 1 with two groups per row crosses 2^32 between its two rows
    big = dm.words(2, 8, SEED, 0, (1 << 31) - 1)
    assert big[1, 0] == dm.philox4x32_10(np.array([0, 1, 0, 0], dtype=np.uint32), [SEED & dm.MASK32, SEED >> 32])[0]
    assert big[0, 7] == dm.philox4x32_10(np.array([0xffffffff, 0, 0, 0], dtype=np.uint32), [SEED & dm.MASK32, SEED >> 32])[3]


def test_apply_multiplies_and_sums_left_to_right():
    rng = np.random.default_rng(3)
    x = rng.standard_normal((5, 10)).astype(np.float32)
    s = [rng.standard_normal((5, 10)).astype(np.float32) for _ in range(3)]
    m = dm.multiplier(5, 10, 0.2, SEED, 9)
    assert set(np.unique(m).tolist()) == {0.0, 1.25}
    assert np.array_equal(dm.apply(x, 0.2, SEED, 9), x * m)
    assert np.array_equal(dm.apply(x, 0.2, SEED, 9, skips=s), ((x * m + s[0]) + s[1]) + s[2])
    # a dropped Inf or NaN is a NaN (Inf * 0), a kept Inf stays Inf
    x[:] = np.inf
    y = dm.apply(x, 0.2, SEED, 9)
    assert np.isnan(y[m == 0]).all() and np.isinf(y[m != 0]).all() and (m == 0).any()
    # the sum starts from +0, as the skip-sum kernel's does: (-0 dropped) + (-0) is +0
    neg = np.full((5, 10), -1.0, dtype=np.float32)
    z = dm.apply(neg, 1, SEED, 9, skips=[np.full((5, 10), -0.0, dtype=np.float32)])
    assert not np.signbit(z).any() and np.signbit(dm.apply(neg, 1, SEED, 9)).all()


def test_entry_point_refuses_on_the_host():
    lib = hip.load_library()

    def call(x=16, s0=None, s1=None, s2=None, y=32, rows=2, frames=6, ld=8, p=0.2, seed=0, call=0, row0=0):
        return lib.nbasr_dropout(x, s0, s1, s2, y, rows, frames, ld, p, seed, call, row0, None), lib.nbasr_last_error()

    for kwargs, code, word in (({'x': None}, -3, b'non-NULL'), ({'y': None}, -3, b'non-NULL'),
                               ({'ld': 4}, -2, b'ld=4'), ({'ld': 6}, -2, b'multiple of 4'), ({'ld': 10}, -2, b'multiple of 4'),
                               ({'x': 20}, -2, b'16-byte'), ({'y': 8}, -2, b'16-byte'), ({'s0': 4}, -2, b'16-byte'),
                               ({'s0': 16, 's1': 16, 's2': 24}, -2, b'16-byte'),
                               ({'p': -0.01}, -1, b'[0, 1]'), ({'p': 1.01}, -1, b'[0, 1]'), ({'p': float('nan')}, -1, b'[0, 1]'),
                               ({'rows': -1}, -1, b'negative size'), ({'frames': -1, 'ld': 0}, -1, b'negative size'),
                               ({'row0': -1}, -1, b'row0=-1'),
                               ({'s1': 16}, -1, b'NULL skip'), ({'s2': 16}, -1, b'NULL skip'), ({'s0': 16, 's2': 16}, -1, b'NULL skip')):
        rc, msg = call(**kwargs)
        assert rc == code and word in msg, (kwargs, rc, msg)
    # nothing to do is no error, whatever the pointers; the other refusals come first
    assert call(rows=0, x=None, y=None)[0] == 0 and call(frames=0, ld=0, x=None, y=None)[0] == 0
    assert call(rows=0, p=2.0)[0] == -1 and call(rows=0, ld=6)[0] == -2
    assert hip.SIGNATURES['nbasr_dropout'][1][8] is __import__('ctypes').c_double and 'nbasr_dropout' in hip._ENQUEUES


class _Library:
    """``nbasr_dropout`` answering on the host: keeps its arguments, returns 0."""

    def __init__(self):
        self.seen = []

    def nbasr_dropout(self, *args):
        self.seen.append(args)
        return 0

    def nbasr_last_error(self):
        return b''


@pytest.fixture
def stub(monkeypatch):
    """The package on a stub library, host tensors let through, and the module's state put back afterwards."""
    lib = _Library()
    monkeypatch.setattr(hip, '_lib', lib)
    monkeypatch.setattr(hip, '_dev', lambda t, name: t.data_ptr())
    monkeypatch.setattr(hip.train, '_dev', lambda t, name: t.data_ptr())
    monkeypatch.setattr(hip.train, '_stream', lambda t: None)
    saved = (dropout._backend, dropout._seed, dropout._calls)
    yield lib
    dropout._backend, dropout._seed, dropout._calls = saved


def test_default_backend_and_use(stub):
    assert dropout.backend() == 'aten' and nb.dropout is dropout
    with dropout.use('hip'):
        assert dropout.backend() == 'hip'
        with dropout.use('aten'):
            assert dropout.backend() == 'aten'
        assert dropout.backend() == 'hip'
    assert dropout.backend() == 'aten'
    dropout.use('hip')                                           # a plain call holds
    assert dropout.backend() == 'hip'
    with pytest.raises(ValueError, match='unknown dropout backend'):
        dropout.use('cuda')
    assert dropout.backend() == 'hip'
    dropout.use('aten')


def test_seed_and_call_counter(stub):
    x = torch.zeros(2, 3, 8)
    dropout.manual_seed(-7)
    assert dropout.get_state() == (-7, 0)
    y = dropout.dropout(x, 0.25)
    assert y.shape == x.shape and dropout.get_state() == (-7, 1)
    dropout.dropout(x, 0.5, True, skips=[x, x])
    assert dropout.get_state() == (-7, 2)
    (x0, s0, s1, s2, y0, rows, frames, ld, p, seed, call, row0, stream), second = stub.seen
    assert (x0, s0, s1, s2, rows, frames, ld, p, seed, call, row0, stream) == (x.data_ptr(), None, None, None, 6, 8, 8, 0.25, -7, 0, 0, None)
    assert y0 not in (x0, None)                                  # a pitched input is only read
    assert second[1] == second[2] == x.data_ptr() and second[3] is None and second[8:12] == (0.5, -7, 1, 0)
    # the identity steps no counter and launches nothing: p == 0, eval
    assert dropout.dropout(x, 0.0) is x and dropout.dropout(x, 0.3, training=False) is x
    assert dropout.get_state() == (-7, 2) and len(stub.seen) == 2
    # a checkpoint resumes onto the same calls
    state = dropout.get_state()
    dropout.dropout(x, 0.25)
    dropout.set_state(state)
    dropout.dropout(x, 0.25)
    assert stub.seen[2][9:11] == stub.seen[3][9:11] == (-7, 2) and dropout.get_state() == (-7, 3)
    dropout.manual_seed(1 << 63)                                 # an unsigned pattern travels as its long long
    dropout.dropout(x, 0.25)
    assert stub.seen[4][9:11] == (-(1 << 63), 0)
    with pytest.raises(ValueError, match='between 0 and 1'):
        dropout.dropout(x, 1.5)
    with pytest.raises(ValueError, match='three skips'):
        dropout.dropout(x, 0.5, True, [x] * 4)
    assert dropout.get_state() == (1 << 63, 1)


def test_unseeded_seed_is_torchs_initial_seed_and_reads_no_generator(stub):
    dropout._seed, dropout._calls = None, 0
    before = torch.get_rng_state()
    assert dropout.get_state() == (torch.initial_seed(), 0)
    dropout.dropout(torch.zeros(1, 1, 4), 0.5)
    assert dropout.get_state() == (torch.initial_seed(), 1) and torch.equal(torch.get_rng_state(), before)


def test_a_slice_of_a_pitched_buffer_is_taken_as_the_buffer(monkeypatch):
    """Only where the buffer is all there: the strides of a pitch of round_up4(frames), a 16-byte aligned start, b * c * ld elements of
    storage behind it.  Everything else goes to the pitching copy of autograd.py."""
    from nb_asr_amd import autograd
    copied = []
    monkeypatch.setattr(autograd, '_pitched', lambda t: copied.append(tuple(t.shape)) or (t, t.shape[2]))
    buf = torch.zeros(2, 3, 12)
    view, frames = dropout._pitched(buf[:, :, :10])
    assert frames == 10 and tuple(view.shape) == (2, 3, 12) and view.data_ptr() == buf.data_ptr() and view.is_contiguous() and not copied
    assert dropout._pitched(buf[:, :, :9])[0].data_ptr() == buf.data_ptr() and not copied            # any frame count of that pitch
    for other in (buf[:, :, 1:11],                                # off the 16-byte groups (and one element short at the end)
                  buf[:, :, :8],                                  # a pitch of 12 is not round_up4(8)
                  buf[:, :, :12],                                 # nothing to do: autograd's own fast path
                  torch.zeros(2, 3, 10),                          # contiguous, unpitched
                  torch.zeros(4 + 2 * 3 * 12 - 2).as_strided((2, 3, 10), (36, 12, 1), 4)):       # the last row's pitch columns are not there
        n = len(copied)
        dropout._pitched(other)
        assert len(copied) == n + 1, tuple(other.shape)


def test_backward_is_the_same_call_on_the_gradient_and_saves_nothing(stub):
    dropout.manual_seed(11)
    x = torch.zeros(2, 3, 8, requires_grad=True)
    s = torch.zeros(2, 3, 8, requires_grad=True)
    y = dropout.dropout(x, 0.25, True, [s])
    assert y.grad_fn.saved_tensors == ()
    dy = torch.ones(2, 3, 8)
    y.backward(dy)
    fwd, bwd = stub.seen
    assert bwd[0] == dy.data_ptr() and bwd[1:4] == (None, None, None) and bwd[5:12] == fwd[5:12] == (6, 8, 8, 0.25, 11, 0, 0)
    assert torch.equal(s.grad, dy) and x.grad.shape == x.shape and dropout.get_state() == (11, 1)
