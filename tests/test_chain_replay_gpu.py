"""A replayed chain depends on nothing its key omits.

Three entry points hand a chain of dependent launches to ``replay_chain`` (csrc/api.cpp): from the third call with one key on, the chain
is an instantiated graph that bakes in every pointer and integer of the launches.  A pointer that the launches read but the key does not
name is a silent error: when the caller comes back with the keyed buffers at the same addresses and THAT buffer elsewhere -- what the
caching allocator does with ``backward.lstm_backward``'s freshly allocated tensors -- the replay reads the old one.

    hip.lstm_backward_step(..., t=-1)          dh_out, w_hh_t, dc, acts, cells, dpre
    hip.lstm_recurrence_packed                 gates_ws, packed_whh, cell_ws, h_out
    hip.lstm_recurrence_frames16_state         gates_ws, packed_whh16, cell_ws, h_out, xcd_ws, h0 (flags = 0 | LSTM_CONTINUE)

Per pointer argument: every buffer is allocated once and stays alive to the end of the module (the swapped-out ones included: nothing
stale is freed, every address read is live memory), four calls with the same buffers (the third captures, the fourth replays), then one
call in which only that argument is another tensor with other contents.  Every call must give what the plain chain gives:

* backward step: the same kernel launched per frame, t = T-1 .. 0 (no cache on that path), bit for bit -- and the float64 evaluation of the
  recurrence in the kernel's header comment, under the tolerance rule of test_backward_edges_gpu.py;
* ``lstm_recurrence_packed``: the one-launch ``lstm_recurrence_seq``, bit for bit (as test_ops_gpu.py does);
* ``lstm_recurrence_frames16_state`` without flags: the resident ``lstm_recurrence_xcd``, bit for bit; with LSTM_CONTINUE, which no other
  kernel implements: the entry point itself on buffers it has never seen -- the first call with a key is always the plain launches.

And an integer: ``batch`` changed over unchanged, large enough buffers gives the new result.

All of it on a side stream -- the legacy default stream refuses a capture, and ``replay_chain`` then keeps to the plain launches.  Before
``cells`` joined the key of the backward chain (csrc/backward.hip), exactly ``test_backward_chain_...[cells]`` failed here: the replay
read the cell states of the tensor it was captured with (max |diff| 0.54 in dpre).
"""
import pytest
import torch

from nb_asr_amd import hip
from test_backward_edges_gpu import check, lstm_bptt_ref, lstm_scan_ref

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
KEEP = []               # every device tensor of this module, to its end: no address comes back to the allocator while a chain may name it
NAN = float('nan')


@pytest.fixture(scope='module')
def side_stream():
    return torch.cuda.Stream(DEV)


@pytest.fixture(autouse=True)
def on_a_side_stream(side_stream):
    """Everything here runs on a stream of its own: the legacy default stream cannot be captured, ``replay_chain`` answers a refused
    capture with the plain launches, and on that stream this file would compare the plain chain with itself."""
    with torch.cuda.stream(side_stream):
        yield
    side_stream.synchronize()


def dev(t):
    t = t.to(DEV).contiguous()
    KEEP.append(t)
    return t


def nans(*shape):
    return dev(torch.full(shape, NAN))


# ---- lstm_backward_step(t = -1) ----------------------------------------------------------------------------------------------------------
BW_H, BW_T, BW_B, BW_LDB = 8, 6, 3, 4
BW_POINTERS = ('dh_out', 'w_hh_t', 'dc', 'acts', 'cells', 'dpre')


def bw_tensor(name, seed):
    """One argument's contents (CPU), (rows, T, ldb) with the utterances innermost; ``dc`` is the value the in/out carry starts from."""
    gen = torch.Generator().manual_seed(seed)
    if name == 'dh_out':
        return torch.randn(BW_H, BW_T, BW_LDB, generator=gen)
    if name == 'w_hh_t':
        return torch.randn(BW_H, 4 * BW_H, generator=gen) * 0.3
    if name == 'dc':
        return torch.randn(BW_H, BW_LDB, generator=gen) * 0.5
    if name == 'dpre':
        return torch.full((4 * BW_H, BW_T, BW_LDB), NAN)
    acts, cells = lstm_scan_ref(torch.randn(4 * BW_H, BW_T, BW_LDB, generator=gen) * 1.5, torch.float32)
    return acts if name == 'acts' else cells


def bw_call(bufs, dc0, batch, chained):
    """Refill the in/out carry and the output, then the whole chain in one call (t = -1) or frame by frame."""
    bufs['dc'].copy_(dc0)
    bufs['dpre'].fill_(NAN)
    args = [bufs[n] for n in BW_POINTERS]
    for t in ([-1] if chained else range(BW_T - 1, -1, -1)):
        hip.lstm_backward_step(*args, batch, t)
    return bufs['dpre'].clone(), bufs['dc'].clone()


def bw_check(bufs, dc0, batch, what):
    """One chained call against the per-frame launches (on output buffers of their own) and against float64."""
    plain = dict(bufs, dc=dev(dc0.clone()), dpre=nans(4 * BW_H, BW_T, BW_LDB))
    want_dpre, want_dc = bw_call(plain, dc0, batch, chained=False)
    dpre, dc = bw_call(bufs, dc0, batch, chained=True)
    assert torch.isfinite(want_dpre).all()
    assert torch.equal(dpre, want_dpre) and torch.equal(dc, want_dc), \
        f'{what}: the chained call differs from the per-frame launches, max |diff| dpre {float((dpre - want_dpre).abs().max()):.3e} dc {float((dc - want_dc).abs().max()):.3e}'
    dh, acts, cells = (bufs[n].cpu()[:, :, :batch] for n in ('dh_out', 'acts', 'cells'))
    ref = [lstm_bptt_ref(dh, bufs['w_hh_t'].cpu(), dc0.cpu()[:, :batch], acts, cells, ty) for ty in (torch.float64, torch.float32)]
    assert torch.equal(dpre[:, :, batch:], torch.zeros_like(dpre[:, :, batch:]))
    check('lstm_backward_chain', what, 'dpre', dpre[:, :, :batch], ref[0][0], ref[1][0])
    check('lstm_backward_chain', what, 'dc', dc[:, :batch], ref[0][1], ref[1][1])


@pytest.mark.parametrize('swapped', BW_POINTERS + ('batch',))
def test_backward_chain_reads_only_what_its_key_names(swapped):
    seed = 100 * (1 + (BW_POINTERS + ('batch',)).index(swapped))
    bufs = {n: dev(bw_tensor(n, seed + i)) for i, n in enumerate(BW_POINTERS)}
    dc0 = dev(bw_tensor('dc', seed + 2))
    for rep in range(4):                                     # the third call captures the chain, the fourth replays it
        bw_check(bufs, dc0, BW_B, f'{swapped}/call{rep}')
    if swapped == 'batch':
        bw_check(bufs, dc0, BW_B - 1, 'batch/2-of-ldb-4')
        return
    other = dev(bw_tensor(swapped, seed + 50))               # another tensor at another address, other contents
    assert other.data_ptr() != bufs[swapped].data_ptr()
    if swapped == 'dc':
        bw_check(dict(bufs, dc=dev(other.clone())), other, BW_B, 'dc/other')
    else:
        bw_check(dict(bufs, **{swapped: other}), dc0, BW_B, f'{swapped}/other')


# ---- the forward recurrences ----------------------------------------------------------------------------------------------------------------
def flat_view(t, *shape):
    """The first prod(shape) elements of ``t``'s storage as ``shape``: the same address, a smaller batch."""
    n = 1
    for s in shape:
        n *= s
    return t.view(-1)[:n].view(*shape)


PK_B, PK_T, PK_H = 5, 4, 12
PK_POINTERS = ('gates', 'packed', 'cell', 'h_out')


def pk_tensor(name, seed, b=PK_B):
    gen = torch.Generator().manual_seed(seed)
    if name == 'gates':
        return dev(torch.randn(PK_T, b, 4 * PK_H, generator=gen))
    if name == 'packed':
        packed = hip.lstm_pack_whh(dev(torch.randn(4 * PK_H, PK_H, generator=gen) * 0.2))
        KEEP.append(packed)
        return packed
    return nans(b, PK_H) if name == 'cell' else nans(b, PK_T, PK_H)


def pk_check(bufs, b, what):
    gates, cell, h_out = flat_view(bufs['gates'], PK_T, b, 4 * PK_H), flat_view(bufs['cell'], b, PK_H), flat_view(bufs['h_out'], b, PK_T, PK_H)
    assert all(v.data_ptr() == bufs[n].data_ptr() for v, n in ((gates, 'gates'), (cell, 'cell'), (h_out, 'h_out')))
    ws = hip.lstm_seq_workspace(b, PK_H, DEV)
    assert ws is not None
    KEEP.append(ws)
    want, want_cell = nans(b, PK_T, PK_H), nans(b, PK_H)
    hip.lstm_recurrence_seq(gates, bufs['packed'], want_cell, want, ws)
    hip.lstm_seq_status(ws)
    cell.fill_(NAN)
    h_out.fill_(NAN)
    hip.lstm_recurrence_packed(gates, bufs['packed'], cell, h_out)
    assert torch.isfinite(want).all()
    assert torch.equal(h_out, want) and torch.equal(cell, want_cell), f'{what}: the chained call differs from the one-launch recurrence'


@pytest.mark.parametrize('swapped', PK_POINTERS + ('batch',))
def test_packed_recurrence_chain_reads_only_what_its_key_names(swapped):
    seed = 7000 + 100 * (PK_POINTERS + ('batch',)).index(swapped)
    bufs = {n: pk_tensor(n, seed + i) for i, n in enumerate(PK_POINTERS)}
    for rep in range(4):
        pk_check(bufs, PK_B, f'{swapped}/call{rep}')
    if swapped == 'batch':
        pk_check(bufs, PK_B - 1, 'batch/4-in-buffers-of-5')
        return
    other = pk_tensor(swapped, seed + 50)
    assert other.data_ptr() != bufs[swapped].data_ptr()
    pk_check(dict(bufs, **{swapped: other}), PK_B, f'{swapped}/other')


FR_B, FR_T, FR_H = 3, 4, 36
FR_POINTERS = ('gates', 'packed', 'cell', 'h_out', 'ws', 'h0')
FR_VARIANTS = {'zero_state': (0, False), 'continue': (hip.LSTM_CONTINUE, False), 'continue_h0': (hip.LSTM_CONTINUE, True)}


def fr_tensor(name, seed, b=FR_B):
    """``cell``: the state a continued call starts from (an output otherwise); ``ws``: the images hold NaN patterns until the call zeroes them."""
    gen = torch.Generator().manual_seed(seed)
    if name == 'gates':
        return dev(torch.randn(FR_T, b, 4 * FR_H, generator=gen))
    if name == 'packed':
        packed = hip.lstm_pack_whh16(dev(torch.randn(4 * FR_H, FR_H, generator=gen) * 0.1))
        KEEP.append(packed)
        return packed
    if name == 'ws':
        return dev(torch.full((hip.lstm_xcd_workspace_bytes(b, FR_H),), 255, dtype=torch.uint8))
    if name == 'h_out':
        return nans(b, FR_T, FR_H)
    return dev(torch.tanh(torch.randn(b, FR_H, generator=gen)))         # cell, h0


def fr_check(bufs, cell0, b, flags, what):
    gates, cell, h_out = flat_view(bufs['gates'], FR_T, b, 4 * FR_H), flat_view(bufs['cell'], b, FR_H), flat_view(bufs['h_out'], b, FR_T, FR_H)
    h0 = None if bufs['h0'] is None else flat_view(bufs['h0'], b, FR_H)
    want, want_cell = nans(b, FR_T, FR_H), dev(flat_view(cell0, b, FR_H).clone())
    if flags == 0:
        hip.lstm_recurrence_xcd(gates, bufs['packed'], want_cell, want, dev(hip.lstm_xcd_workspace(b, FR_H, DEV)))
    else:
        # buffers no chain has seen: the plain launches.  (Every earlier tensor is alive, so each of these addresses is new.)
        hip.lstm_recurrence_frames16_state(dev(gates.clone()), dev(bufs['packed'].clone()), want_cell, want, fr_tensor('ws', 0, b),
                                           None if h0 is None else dev(h0.clone()), flags)
    cell.copy_(flat_view(cell0, b, FR_H))
    h_out.fill_(NAN)
    hip.lstm_recurrence_frames16_state(gates, bufs['packed'], cell, h_out, bufs['ws'], h0, flags)
    assert torch.isfinite(want).all() and torch.isfinite(want_cell).all()
    assert torch.equal(h_out, want) and torch.equal(cell, want_cell), f'{what}: the chained call differs from the plain chain'


FR_CASES = [(v, p) for v in FR_VARIANTS for p in FR_POINTERS + ('batch',) if p != 'h0' or FR_VARIANTS[v][1]]


@pytest.mark.parametrize('variant,swapped', FR_CASES)
def test_frames16_chain_reads_only_what_its_key_names(variant, swapped):
    flags, with_h0 = FR_VARIANTS[variant]
    seed = 9000 + 1000 * list(FR_VARIANTS).index(variant) + 100 * (FR_POINTERS + ('batch',)).index(swapped)
    bufs = {n: fr_tensor(n, seed + i) for i, n in enumerate(FR_POINTERS)}
    if not with_h0:
        bufs['h0'] = None
    cell0 = dev(bufs['cell'].clone())
    for rep in range(4):
        fr_check(bufs, cell0, FR_B, flags, f'{variant}/{swapped}/call{rep}')
    if swapped == 'batch':
        fr_check(bufs, cell0, FR_B - 1, flags, f'{variant}/batch/2-in-buffers-of-3')
        return
    other = fr_tensor(swapped, seed + 50)
    assert other.data_ptr() != bufs[swapped].data_ptr()
    if swapped == 'cell':
        fr_check(dict(bufs, cell=dev(other.clone())), other, FR_B, flags, f'{variant}/cell/other')
    else:
        fr_check(dict(bufs, **{swapped: other}), cell0, FR_B, flags, f'{variant}/{swapped}/other')
