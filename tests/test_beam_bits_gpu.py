"""The CTC prefix beam search (ctc_decode.hip) and the CTC loss (ctc_loss.hip), pinned to the bit: SHA-256 of what the kernels write,
compared with a recording made from the kernels before their shared steps were folded into one copy each and the loss left the decode
file (tests/golden/beam_bits.json).  No tolerance: one wavefront per utterance, no atomics, every sum in one fixed order (the gradient's
per-class sum walks the label positions serially), so a digest can only move if behaviour did.  Chunked against whole, peek against
push-then-finish and timed against untimed all come from the same file and would move together; this recording would not.

The inputs are lp = -sharp * keyed_uniform in [0, 1), one float32 product per element and no host log_softmax, so their bits do not
depend on the torch build.  Only what the kernels define is digested: whole-search, finish and peek outputs whole (every element is
written); a step's committed / partial rows (and their frame rows) cut to their counts, and the (3, B) counts; the state tensor whole
after every step -- it is allocated zeroed and exactly ctc_beam_stream_state_bytes long, so unwritten pool nodes are zero and the record
layout is pinned too.  Neither the `ids` workspace nor the peek's scratch is digested.  Every beam case runs untimed and timed.

    W1  whole search, width 3, 5 classes, lengths (24, 0, 11): a zero-length utterance; a narrow beam where prefixes leave and are
        created again; n_live < width in the first frames
    W2  whole search, width 32, 64 classes, cutoff 10: the prune pre-pass, all 64 lanes, the width limit
    W3  whole search, width 12, 49 classes, lp in multiples of 0.25: exact ties reach the slot tie-break
    S1  W1's input in chunks of (1, 0, 7, 16) frames with the chunk lengths that follow from W1's lengths: one utterance takes nothing,
        one ends inside a chunk; then finish with ld = the longest suffix and with ld = 1 (the k < ld guard)
    S2  W3's input in chunks of 13: commits, and a compaction of more than 64 nodes (the 64-wide renumbering takes a second pass;
        asserted: a committing step leaves more than 64 kept nodes)
    S3  a step whose pool is one node too small for the chunk: usage -1, counts 0, the state as it was
    K1  peeks at S1's state after its second and third step, with 5 frames and with none, and at S2's state after its first step with
        6 frames: the timed peek's rule for the first lcp columns (asserted: some peek has several live rows with a common part); no
        peek changes the state
    L   hip.ctc_loss and hip.ctc_loss_grad, 2 utterances of 12 frames, 5 classes, targets of length 3 and 0

    python tests/test_beam_bits_gpu.py --record        # rewrites the fixture from the code as it is
"""
import hashlib
import json
import pathlib
import sys

import numpy as np
import pytest
import torch

REPO = pathlib.Path(__file__).resolve().parent.parent
if str(REPO) not in sys.path:
    sys.path.insert(0, str(REPO))

from nb_asr_amd import hip                              # noqa: E402
from nb_asr_amd.utils import keyed_uniform              # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
FIXTURE = REPO / 'tests' / 'golden' / 'beam_bits.json'

# name: (batch, frames, classes, width, cutoff_top_n, sharp, quantum or None, lengths or None)
INPUTS = {
    'W1': (3, 24, 5, 3, 40, 6.0, None, (24, 0, 11)),
    'W2': (2, 12, 64, 32, 10, 8.0, None, None),
    'W3': (2, 40, 49, 12, 40, 40.0, 0.25, None),
}
# name: (input, chunk sizes, pool_nodes)
STREAMS = {'S1': ('W1', (1, 0, 7, 16), 80), 'S2': ('W3', (13, 13, 13, 1), 640)}
S3_FRAMES = 8                                           # of W1's input, every utterance whole: 1 + 3 * 8 + 1 nodes needed, 3 * 8 + 1 given
# (stream, steps taken before the peek, frames peeked)
PEEKS = (('S1', 2, 5), ('S1', 2, 0), ('S1', 3, 5), ('S1', 3, 0), ('S2', 1, 6))
CASES = [f'{name}-{kind}' for name in ('W1', 'W2', 'W3', 'S1', 'S2', 'S3', 'K1') for kind in ('plain', 'timed')] + ['L']


def digest(*tensors):
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.contiguous().view(torch.uint8).cpu().numpy().tobytes())
    return h.hexdigest()


def log_probs(name):
    """lp (batch, frames, classes) float32 on the host, and the utterances' lengths (None: all frames)."""
    b, t, c, _, _, sharp, quantum, lengths = INPUTS[name]
    lp = np.float32(-sharp) * keyed_uniform(f'beam_bits/{name}', 0, (b, t, c), 0.0, 1.0)
    if quantum:
        lp = np.round(lp / np.float32(quantum)) * np.float32(quantum)
    return torch.from_numpy(lp.astype(np.float32)), lengths


def ints(values):
    return None if values is None else torch.tensor(values, dtype=torch.int32, device=DEV)


def named(outs, timed):
    return dict(zip(('beams', 'scores', 'steps', 'lens') if timed else ('beams', 'scores', 'lens'), (digest(t) for t in outs)))


def whole(name, timed):
    _, _, _, width, cutoff, _, _, _ = INPUTS[name]
    lp, lengths = log_probs(name)
    return named(hip.ctc_beam_search(lp.to(DEV), ints(lengths), width, 0, cutoff, timesteps=timed), timed)


def fresh_state(batch, width, pool_nodes, timed):
    state = torch.zeros(hip.ctc_beam_stream_state_bytes(batch, width, pool_nodes, timed), dtype=torch.uint8, device=DEV)
    hip.ctc_beam_stream_init(state, batch, width, pool_nodes, timed)
    return state


def chunk_of(lp, lengths, at, n):
    """Frames [at, at + n) on the device, and how many of them belong to each utterance."""
    chunk_lengths = None if lengths is None else ints([min(max(v - at, 0), n) for v in lengths])
    return lp[:, at:at + n].contiguous().to(DEV), chunk_lengths


def step(chunk, chunk_lengths, state, width, pool_nodes, cutoff, timed):
    """One step's digests (rows cut to their counts), and the counts on the host."""
    *rows, counts = hip.ctc_beam_stream_step(chunk, chunk_lengths, state, width, pool_nodes, 0, cutoff, timesteps=timed)
    counts_host = counts.cpu()
    out = {'counts': digest(counts), 'state': digest(state)}
    for what, row, n in zip(('committed', 'partial', 'committed_frames', 'partial_frames'), rows, (0, 1, 0, 1)):
        out[what] = digest(*(row[i, : int(counts_host[n, i])] for i in range(row.shape[0])))
    return out, counts_host


def stream(name, timed, steps=None):
    """Feed the first ``steps`` chunks (None: all) of a stream.  -> (digests per step, state, frames fed, last step's counts)."""
    source, sizes, pool_nodes = STREAMS[name]
    b, _, _, width, cutoff, _, _, _ = INPUTS[source]
    lp, lengths = log_probs(source)
    state = fresh_state(b, width, pool_nodes, timed)
    out, at, counts, second_pass = {}, 0, None, False
    for i, n in enumerate(sizes[:steps]):
        out[f'step{i}'], counts = step(*chunk_of(lp, lengths, at, n), state, width, pool_nodes, cutoff, timed)
        assert int(counts[2].min()) >= 1, f'{name}: step {i} was refused'
        print(f'{name} step {i}: committed {counts[0].tolist()} partial {counts[1].tolist()} usage {counts[2].tolist()}')
        second_pass |= bool(((counts[0] > 0) & (counts[2] > 65)).any())       # usage = 1 + kept nodes
        at += n
    if name == 'S2' and steps is None:
        assert second_pass, 'S2: no committing step keeps more than 64 nodes, the renumbering never takes a second pass'
    return out, state, at, counts


def streamed(name, timed):
    source, _, pool_nodes = STREAMS[name]
    b, _, _, width, _, _, _, _ = INPUTS[source]
    out, state, _, _ = stream(name, timed)
    before = digest(state)
    lens = hip.ctc_beam_stream_finish(state, b, width, pool_nodes, 1, timesteps=timed)[-1]
    longest = max(int(lens.max()), 1)
    out['finish'] = named(hip.ctc_beam_stream_finish(state, b, width, pool_nodes, longest, timesteps=timed), timed)
    if name == 'S1':
        assert longest > 1, 'S1: no suffix longer than ld = 1, the k < ld guard is not reached'
        out['finish_ld1'] = named(hip.ctc_beam_stream_finish(state, b, width, pool_nodes, 1, timesteps=timed), timed)
    assert digest(state) == before, f'{name}: finish wrote to the state'
    return out


def refused(timed):
    b, _, _, width, cutoff, _, _, _ = INPUTS['W1']
    pool_nodes = width * S3_FRAMES + 1
    lp, _ = log_probs('W1')
    state = fresh_state(b, width, pool_nodes, timed)
    before = digest(state)
    out, counts = step(*chunk_of(lp, None, 0, S3_FRAMES), state, width, pool_nodes, cutoff, timed)
    assert counts.tolist() == [[0] * b, [0] * b, [-1] * b], counts.tolist()
    assert out['state'] == before, 'S3: a refused step changed the state'
    return out


def shared_prefix(beams, lens):
    """The longest non-empty token prefix that two or more live rows of one utterance share, over the utterances."""
    best = 0
    for rows, n in zip(beams.cpu(), lens.cpu()):
        live = [rows[r, : int(n[r])].tolist() for r in range(rows.shape[0]) if int(n[r]) >= 0]
        k = 0
        while len(live) > 1 and all(len(x) > k and x[k] == live[0][k] for x in live):
            k += 1
        best = max(best, k)
    return best


def peeked(timed):
    out, common = {}, {}
    for name, steps, n in PEEKS:
        source, _, pool_nodes = STREAMS[name]
        _, _, _, width, cutoff, _, _, _ = INPUTS[source]
        lp, lengths = log_probs(source)
        _, state, at, counts = stream(name, timed, steps)
        before = digest(state)
        ld = max(int(counts[2].max()) - 1 + n, 1)                     # a frame lengthens a suffix by at most one token
        outs = hip.ctc_beam_stream_peek(*chunk_of(lp, lengths, at, n), state, width, pool_nodes, ld, 0, cutoff, timesteps=timed)
        out[f'{name}/{steps}/{n}'] = named(outs, timed)
        assert digest(state) == before, f'K1: the peek {name}/{steps}/{n} changed the state'
        common[f'{name}/{steps}/{n}'] = shared_prefix(outs[0], outs[-1])
    print(f'K1: common suffix prefix of the live rows {common}')
    assert max(common.values()) > 0, 'K1: no peek has several live rows with a common part, the first-lcp-columns rule is not reached'
    return out


def loss():
    lp = (np.float32(-3.0) * keyed_uniform('beam_bits/L', 0, (2, 12, 5), 0.0, 1.0)).astype(np.float32)
    args = torch.from_numpy(lp).to(DEV), ints([12, 9]), ints([[1, 3, 3], [2, 4, 1]]), ints([3, 0])
    per_length, grad = hip.ctc_loss_grad(*args)
    return {'loss': digest(hip.ctc_loss(*args)), 'loss_per_length': digest(hip.ctc_loss(*args, divide_by_length=True)),
            'grad_loss': digest(per_length), 'grad': digest(grad)}


def run(case):
    name, _, kind = case.partition('-')
    timed = kind == 'timed'
    if name in INPUTS:
        return whole(name, timed)
    if name in STREAMS:
        return streamed(name, timed)
    return {'S3': refused, 'K1': peeked}[name](timed) if name != 'L' else loss()


@pytest.fixture(scope='module')
def pinned():
    return json.loads(FIXTURE.read_text())


def test_fixture_lists_exactly_the_cases(pinned):
    assert sorted(pinned) == sorted(CASES)


@pytest.mark.parametrize('case', CASES)
def test_beam_bits_are_the_recorded_ones(pinned, case):
    got = run(case)
    print(f'{case}: {got}')
    assert got == pinned[case]


if __name__ == '__main__':
    if sys.argv[1:] != ['--record']:
        raise SystemExit(__doc__)
    FIXTURE.write_text('{\n' + ',\n'.join(f'{json.dumps(case)}: {json.dumps(run(case))}' for case in CASES) + '\n}\n')
    print(f'wrote {len(CASES)} cases to {FIXTURE}')
