"""Streaming beam decode without a GPU: the C ABI of nbasr_ctc_beam_stream_* (bound with the header's signatures, arguments refused on
the host), and the committed-prefix argument it rests on, checked on the CPU oracle independently of the kernel: the longest common
token prefix of the live beams after frame t is a prefix of every beam after every later frame."""
import pytest
import torch

from nb_asr_amd import hip
from nbasr_header import declarations
from oracle import decode_oracle as oracle

NAMES = ('nbasr_ctc_beam_stream_state_bytes', 'nbasr_ctc_beam_stream_workspace_bytes', 'nbasr_ctc_beam_stream_init',
         'nbasr_ctc_beam_stream_step', 'nbasr_ctc_beam_stream_finish')


@pytest.mark.parametrize('name', NAMES)
def test_symbols_are_bound_with_the_header_signature(name):
    """Declared, and loaded with the binding's types; that those are the header's is test_abi.py's check of every symbol."""
    assert name in declarations() and getattr(hip.load_library(), name).argtypes == hip.SIGNATURES[name][1]


def _err(lib):
    return lib.nbasr_last_error()


def test_step_refuses_bad_arguments_on_the_host():
    lib = hip.load_library()
    p = 16                                            # a non-NULL, 8-byte aligned stand-in: every case is refused before a launch
    #      log_probs, lengths, state, ws, committed, c_counts, partial, p_counts, usage, batch, frames, classes, width, blank, top_n, pool
    ok = [p, None, p, p, p, p, p, p, p, 2, 5, 49, 12, 0, 40, 100]

    def step(**kw):
        a = list(ok)
        for k, v in kw.items():
            a[{'state': 2, 'ws': 3, 'committed': 4, 'usage': 8, 'classes': 11, 'width': 12, 'blank': 13, 'pool': 15}[k]] = v
        return lib.nbasr_ctc_beam_stream_step(*a, None)
    assert step(state=None) == -3 and b'NULL pointer' in _err(lib)
    assert step(ws=None) == -3 and b'NULL pointer' in _err(lib)
    assert step(usage=None) == -3 and b'NULL pointer' in _err(lib)
    assert step(width=33) == -1 and b'beam_width=33' in _err(lib)
    assert step(classes=65) == -1 and b'classes=65' in _err(lib)
    assert step(blank=49) == -1 and b'blank=49' in _err(lib)
    assert step(pool=0) == -1 and b'pool_nodes=0' in _err(lib)
    assert step(state=20) == -2 and b'8-byte aligned' in _err(lib)


def test_init_and_finish_refuse_bad_arguments_on_the_host():
    lib = hip.load_library()
    assert lib.nbasr_ctc_beam_stream_init(None, 2, 12, 100, None) == -3 and b'NULL pointer' in _err(lib)
    assert lib.nbasr_ctc_beam_stream_init(16, 2, 33, 100, None) == -1 and b'beam_width=33' in _err(lib)
    assert lib.nbasr_ctc_beam_stream_init(12, 2, 12, 100, None) == -2 and b'8-byte aligned' in _err(lib)
    assert lib.nbasr_ctc_beam_stream_finish(None, 16, 16, 16, 4, 2, 12, 100, None) == -3 and b'NULL pointer' in _err(lib)
    assert lib.nbasr_ctc_beam_stream_finish(16, 16, 16, None, 4, 2, 12, 100, None) == -3
    assert lib.nbasr_ctc_beam_stream_finish(16, 16, 16, 16, 4, 2, 33, 100, None) == -1 and b'beam_width=33' in _err(lib)
    assert lib.nbasr_ctc_beam_stream_finish(36, 16, 16, 16, 4, 2, 12, 100, None) == -2 and b'8-byte aligned' in _err(lib)
    # nothing to do for an empty batch; sizes of a bad shape are 0
    assert lib.nbasr_ctc_beam_stream_init(None, 0, 12, 100, None) == 0
    assert lib.nbasr_ctc_beam_stream_state_bytes(2, 33, 100) == 0 and lib.nbasr_ctc_beam_stream_state_bytes(2, 12, 0) == 0


def test_state_bytes_grow_with_the_pool_only():
    lib = hip.load_library()
    a, b = lib.nbasr_ctc_beam_stream_state_bytes(1, 12, 100), lib.nbasr_ctc_beam_stream_state_bytes(1, 12, 300)
    assert a % 8 == 0 and b - a == 200 * 8                              # one int2 (parent, class) per pool node
    assert lib.nbasr_ctc_beam_stream_state_bytes(5, 12, 100) == 5 * a
    assert lib.nbasr_ctc_beam_stream_state_bytes(1, 7, 100) % 8 == 0        # odd widths keep every record 8-byte aligned
    assert lib.nbasr_ctc_beam_stream_workspace_bytes(2, 10, 49, 100) == 2 * 100 * 4 + 2 * 10 * 49 * 4


def _lcp(seqs):
    out = []
    for toks in zip(*seqs):
        if any(t != toks[0] for t in toks):
            break
        out.append(toks[0])
    return out


@pytest.mark.parametrize('seed,frames,classes,width,sharp', [
    (0, 30, 5, 3, 1.0), (1, 30, 5, 4, 0.3), (2, 40, 7, 12, 2.0), (3, 25, 3, 2, 1.0), (4, 30, 49, 12, 3.0), (5, 24, 4, 1, 1.0)])
def test_committed_prefix_theorem_on_the_oracle(seed, frames, classes, width, sharp):
    gen = torch.Generator().manual_seed(seed)
    lp = torch.randn(frames, classes, generator=gen) * sharp
    lp[::3, 0] += 1.5
    lp = torch.log_softmax(lp, dim=1).numpy()
    live = [[tok for tok, _ in oracle.ctc_beam_search(lp[:t], width)] for t in range(frames + 1)]
    commits = [_lcp(beams) for beams in live]
    for t in range(frames + 1):
        for later in range(t, frames + 1):
            for tok in live[later]:
                assert tok[: len(commits[t])] == commits[t], (t, later, commits[t], tok)
        if t:
            assert commits[t][: len(commits[t - 1])] == commits[t - 1]         # committed tokens never change
