"""CTC forced alignment without a GPU: the C ABI's surface and refusals, and the numpy statement of the definition
(tests/ctc_align_model.py) against brute force over every labelling."""
import ctypes
import itertools
import pathlib
import re

import numpy as np
import pytest
import torch

import ctc_align_model as model
from nb_asr_amd import hip
from oracle import decode_oracle

HEADER = pathlib.Path(__file__).resolve().parent.parent / 'include' / 'nbasr.h'
NAMES = ('nbasr_ctc_align_workspace_bytes', 'nbasr_ctc_forced_align')


def test_header_binding_and_library_agree(built_library):
    code = re.sub(r'/\*.*?\*/', '', HEADER.read_text(), flags=re.S)
    lib = ctypes.CDLL(str(built_library))
    for name in NAMES:
        assert re.search(r'\b' + name + r'\s*\(', code), name
        assert name in hip.SIGNATURES
        assert hasattr(lib, name), name
    assert len(hip.SIGNATURES['nbasr_ctc_forced_align'][1]) == 16 and len(hip.SIGNATURES['nbasr_ctc_align_workspace_bytes'][1]) == 3
    comment = HEADER.read_text().split('nbasr_ctc_forced_align:')[1].split('*/')[0]
    for words in ('smallest step', 'on a tie', 'increasing frame order', '-inf', 'NaN'):
        assert words in comment, words


def test_workspace_size():
    size = hip.load_library().nbasr_ctc_align_workspace_bytes
    for bad in ((0, 10, 4), (-1, 10, 4), (2, 0, 4), (2, -3, 4), (2, 10, -1), (2, 10, 1025)):
        assert size(*bad) == 0, bad
    # the documented layout: per utterance and frame, W words for each of 64 lanes; 16 two-bit back-pointers to a word, a lane owns every 64th position
    for batch, frames, ld in ((1, 1, 0), (3, 7, 1), (64, 250, 40), (2, 11, 511), (2, 11, 512), (1, 5, 1023), (1, 1030, 1024)):
        positions = 2 * ld + 1
        per_lane = -(-positions // 64)
        words = -(-per_lane // 16)
        assert size(batch, frames, ld) == batch * frames * words * 64 * 4, (batch, frames, ld)
        assert size(batch, frames, ld) * 8 >= batch * frames * positions * 2            # two bits for every cell


def test_refusals_without_a_device():
    lib = hip.load_library()
    p = 16                                                                               # stands for a device address: refused calls touch nothing
    def call(log_probs=p, lengths=p, targets=p, target_lengths=p, ws=p, scores=p, path=p, starts=p, ends=p, token_scores=p,
             batch=1, frames=10, classes=5, ld_targets=3, blank=0):
        return lib.nbasr_ctc_forced_align(log_probs, lengths, targets, target_lengths, ws, scores, path, starts, ends, token_scores,
                                          batch, frames, classes, ld_targets, blank, None)
    for null in ('log_probs', 'lengths', 'targets', 'target_lengths', 'ws', 'scores', 'path', 'starts', 'ends', 'token_scores'):
        assert call(**{null: None}) == -3 and b'nbasr_ctc_forced_align: NULL' in lib.nbasr_last_error(), null
    assert call(ld_targets=1025) == -1 and b'at most 1024 labels' in lib.nbasr_last_error()
    assert call(blank=5) == -1 and b'blank=5' in lib.nbasr_last_error()
    assert call(blank=-1) == -1 and call(classes=0) == -1 and b'classes=0' in lib.nbasr_last_error()
    assert call(frames=-1) == -1 and call(batch=-1) == -1
    assert call(batch=0) == 0
    assert call(batch=0, log_probs=None, lengths=None, scores=None) == 0                 # nothing to launch, nothing needed


def _labellings(frames, classes):
    return itertools.product(range(classes), repeat=frames)


def _cases():
    rng = np.random.default_rng(7)
    for frames in range(1, 7):
        for n_lab in range(0, 3):
            for target in itertools.product((1, 2), repeat=n_lab):
                for blank in (0,):
                    yield frames, list(target), blank, -rng.exponential(1.5, size=(frames, 3))
    # another blank, and ties: values from a small exact set
    for frames in (3, 5, 6):
        for target in ([0], [0, 1], [1, 1], [1, 0]):
            yield frames, target, 2, -rng.integers(0, 4, size=(frames, 3)) * 0.5


def test_oracle_against_brute_force():
    """Every (T <= 6, L <= 2, 3 classes) case: the float64 score is the maximum over all labellings that collapse to the target, and the
    path is one of the maximisers."""
    checked = 0
    for frames, target, blank, lp in _cases():
        best, winners = -np.inf, []
        for lab in _labellings(frames, 3):
            if model.collapse(lab, blank) != target:
                continue
            s = model.path_score(lp, lab)[0]
            if s > best:
                best, winners = s, [lab]
            elif s == best:
                winners.append(lab)
        got = model.forced_align(lp, frames, target + [999], len(target), blank, np.float64)
        if not winners:
            assert got['score'] == -np.inf and (got['path'] == -1).all() and (got['starts'] == -1).all()
            continue
        assert got['score'] == pytest.approx(best, rel=1e-14, abs=1e-14)
        path = tuple(int(c) for c in got['path'])
        assert model.collapse(path, blank) == target
        assert model.path_score(lp, path)[0] == pytest.approx(best, rel=1e-14, abs=1e-14)
        if all(float(v) == round(float(v) * 2) / 2 for v in lp.reshape(-1)):             # exact sums: the path is literally a maximiser
            assert path in winners
        for j, lab in enumerate(target):                                                 # spans tile the label frames
            assert all(path[t] == lab for t in range(got['starts'][j], got['ends'][j])) and got['starts'][j] < got['ends'][j]
        assert got['starts'][len(target)] == -1 and got['token_scores'][len(target)] == 0
        checked += 1
    assert checked > 40


def test_tie_rule_by_hand():
    # all-zero log-probs: every path scores 0.  Every cell that was reachable a frame earlier stays, so walking back the path stays on a
    # position down to the first frame that reached it: every label is entered as early as it can be, and the end is on the last label,
    # never on the trailing blank.
    got = model.forced_align(np.zeros((4, 3)), 4, [1, 2], 2, 0, np.float32)
    assert got['score'] == 0 and got['path'].tolist() == [1, 2, 2, 2]
    assert got['starts'].tolist() == [0, 1] and got['ends'].tolist() == [1, 4]
    got = model.forced_align(np.zeros((4, 3)), 4, [1, 1], 2, 0, np.float32)           # a repeat needs its blank
    assert got['path'].tolist() == [1, 0, 1, 1]
    assert model.forced_align(np.zeros((2, 3)), 2, [1, 1], 2, 0, np.float32)['score'] == -np.inf
    assert np.isnan(model.forced_align(np.zeros((2, 3)), 2, [0, 1], 1, 0, np.float32)['score'])     # blank as a label
    assert np.isnan(model.forced_align(np.zeros((2, 3)), 2, [3, 1], 1, 0, np.float32)['score'])
    assert model.forced_align(np.zeros((2, 3)), 2, [3, 1], 0, 0, np.float32)['score'] == 0            # beyond L: never read
    assert model.forced_align(np.zeros((2, 3)), 0, [3, 1], 0, 0, np.float32)['score'] == 0
    assert model.forced_align(np.zeros((2, 3)), 0, [1, 1], 1, 0, np.float32)['score'] == -np.inf


def test_best_path_never_beats_the_total_likelihood():
    """The float64 score of the best path <= the log-likelihood of the transcript (all paths), taken from the CPU CTC oracle of the loss tests."""
    rng = np.random.default_rng(11)
    b, frames, classes, ld = 12, 30, 7, 6
    lp = torch.log_softmax(torch.from_numpy(rng.normal(size=(b, frames, classes)) * 2.0), dim=2)
    lengths = rng.integers(14, frames + 1, size=b)
    target_lengths = rng.integers(0, ld + 1, size=b)
    targets = rng.integers(1, classes, size=(b, ld))
    nll = decode_oracle.ctc_loss(lp, lengths, targets, target_lengths, reduce=False) * torch.as_tensor(lengths)
    scores = model.align_batch(lp.numpy(), lengths, targets, target_lengths, 0, np.float64)[0]
    assert np.isfinite(scores).all()
    total = -nll.numpy()
    assert (scores <= total + 1e-12 * np.abs(total)).all()
    assert (scores >= total - lengths * np.log(3.0) - 1e-9).all()         # at most 3 predecessors per frame: the best path holds at least 3^-len of the mass
