"""CTC forced alignment on the device (ctc.forced_align, ctc.align; nbasr_ctc_forced_align): every output equals the float32 statement of
the definition (ctc_align_model.py, anchored on brute force by test_ctc_align_host.py) bit for bit -- the score as its bit pattern, NaN and
-inf included -- and every finite result has the properties of an alignment and lies within fp32 rounding of the float64 optimum."""
import numpy as np
import pytest
import torch

import ctc_align_model as model
import nb_asr_amd as nb
from nb_asr_amd import ctc
from nb_asr_amd.weights import keyed_fill_, keyed_input

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
CLASSES = 49


def _log_probs(rng, b, frames, classes=CLASSES):
    return torch.log_softmax(torch.from_numpy(rng.normal(size=(b, frames, classes)).astype(np.float32) * 2.0), dim=2).numpy()


def _labels(rng, n, classes=CLASSES, blank=0, repeats=True):
    """n random labels (never the blank); ``repeats=False``: no two adjacent labels equal."""
    pool = np.array([c for c in range(classes) if c != blank])
    out = rng.choice(pool, size=n)
    if not repeats:
        for i in range(1, n):
            while out[i] == out[i - 1]:
                out[i] = rng.choice(pool)
    return out.astype(np.int32)


def _device(lp, lengths, targets, target_lengths, blank=0):
    """One ``ctc.forced_align`` call -> numpy (scores, path, starts, ends, token_scores), the kernel's order."""
    out = ctc.forced_align(torch.from_numpy(np.ascontiguousarray(lp)).to(DEV), torch.as_tensor(np.asarray(lengths)), torch.from_numpy(np.asarray(targets, dtype=np.int32)).to(DEV),
                           torch.as_tensor(np.asarray(target_lengths)), blank=blank)
    assert out.score.dtype == torch.float32 and out.token_scores.dtype == torch.float32
    assert out.path.dtype == out.starts.dtype == out.ends.dtype == torch.int32
    return tuple(t.cpu().numpy() for t in (out.score, out.path, out.starts, out.ends, out.token_scores))


def _assert_bits(got, want, what=''):
    for name, g, w in zip(('score', 'path', 'starts', 'ends', 'token_scores'), got, want):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape, g.dtype, w.dtype)
        assert np.array_equal(g.view(np.int32), w.view(np.int32)), (what, name, g, w)


def _check(lp, lengths, targets, target_lengths, blank=0, what=''):
    """Device = float32 model bit for bit; the properties of every finite result; the float64 bounds where lp <= 0.  Returns the device's outputs."""
    lengths, target_lengths = np.asarray(lengths), np.asarray(target_lengths)
    got = _device(lp, lengths, targets, target_lengths, blank)
    _assert_bits(got, model.align_batch(lp, lengths, targets, target_lengths, blank, np.float32), what)
    scores, path, starts, ends, token_scores = got
    frames = lp.shape[1]
    for b in range(lp.shape[0]):
        n, n_lab = min(max(int(lengths[b]), 0), frames), min(max(int(target_lengths[b]), 0), targets.shape[1])
        if not np.isfinite(scores[b]):
            assert (path[b] == -1).all() and (starts[b] == -1).all() and (ends[b] == -1).all() and (token_scores[b] == 0).all(), (what, b)
            continue
        want = [int(c) for c in targets[b][:n_lab]]
        assert model.collapse(path[b], blank) == want and (path[b][n:] == -1).all() and (path[b][:n] >= 0).all(), (what, b)
        covered = np.zeros(frames, bool)
        for j in range(n_lab):                                   # spans: non-empty, in order, exactly the path's label frames
            assert 0 <= starts[b][j] < ends[b][j] <= n and (path[b][starts[b][j]:ends[b][j]] == want[j]).all(), (what, b, j)
            assert j + 1 == n_lab or ends[b][j] <= starts[b][j + 1], (what, b, j)
            covered[starts[b][j]:ends[b][j]] = True
        assert np.array_equal(covered[:n], path[b][:n] != blank), (what, b)
        assert (starts[b][n_lab:] == -1).all() and (ends[b][n_lab:] == -1).all() and (token_scores[b][n_lab:] == 0).all(), (what, b)
        if n == 0 or not (lp[b, :n] <= 0).all():
            continue
        best = model.forced_align(lp[b], n, targets[b], n_lab, blank, np.float64)['score']
        along, mag = model.path_score(lp[b].astype(np.float64), path[b])
        print(f'{what} utterance {b}: len {n} L {n_lab} score {scores[b]!r} float64 optimum - device path {best - along:.3e} '
              f'(bound {2 * n * 2.0 ** -24 * mag:.3e}) |device score - its path in float64| {abs(float(scores[b]) - along):.3e} (bound {n * 2.0 ** -24 * mag:.3e})')
        assert 0 <= best - along <= 2 * n * 2.0 ** -24 * mag, (what, b, best, along)
        assert abs(float(scores[b]) - along) <= n * 2.0 ** -24 * mag, (what, b, scores[b], along)
    return got


def test_smallest_shapes():
    rng = np.random.default_rng(1)
    for n, n_lab in ((1, 0), (1, 1), (2, 1), (5, 2)):             # the call's shapes are the utterance's own: frames = len, ld_targets = L
        _check(_log_probs(rng, 1, n), [n], _labels(rng, n_lab).reshape(1, n_lab), [n_lab], what=f'alone {n},{n_lab}')
    lp = _log_probs(rng, 4, 5)
    got = _check(lp, [1, 1, 2, 5], np.stack([_labels(rng, 2) for _ in range(4)]), [0, 1, 1, 2], what='smallest batch')
    assert np.isfinite(got[0]).all() and got[1][0].tolist() == [0, -1, -1, -1, -1]


@pytest.mark.parametrize('n_lab,n', [(31, 62), (32, 64), (64, 128), (600, 700)])
def test_lane_boundaries(n_lab, n):
    """S = 63, 65, 129: below, across and two rounds of the 64 lanes; L = 600: more than 16 positions per lane, a second packed word."""
    rng = np.random.default_rng(n_lab)
    got = _check(_log_probs(rng, 2, n), [n, n - 3], np.stack([_labels(rng, n_lab), _labels(rng, n_lab, repeats=False)]), [n_lab, n_lab], what=f'L {n_lab}')
    assert np.isfinite(got[0]).all()


def test_longest_transcript():
    """L = 1024 at len = 1030: 2 049 positions, a third packed word for lane 0 alone."""
    rng = np.random.default_rng(1024)
    got = _check(_log_probs(rng, 1, 1030), [1030], _labels(rng, 1024, repeats=False).reshape(1, -1), [1024], what='L 1024')
    assert np.isfinite(got[0]).all()


def test_tight_paths():
    rng = np.random.default_rng(3)
    distinct = (rng.permutation(48)[:40] + 1).astype(np.int32)
    got = _check(_log_probs(rng, 1, 40), [40], distinct.reshape(1, -1), [40], what='len = L')
    assert got[1][0].tolist() == distinct.tolist() and got[2][0].tolist() == list(range(40))          # one path, no blanks
    repeated = np.array([[3, 3, 5, 5, 5, 2, 7, 7]], dtype=np.int32)                                     # 8 labels, 4 adjacent repeats
    got = _check(_log_probs(rng, 1, 12), [12], repeated, [8], what='len = L + repeats')
    assert got[1][0].tolist() == [3, 0, 3, 5, 0, 5, 0, 5, 2, 7, 0, 7]
    got = _check(_log_probs(rng, 1, 12), [11], repeated, [8], what='one frame less')
    assert got[0][0] == -np.inf
    got = _check(_log_probs(rng, 1, 11), [11], repeated, [8], what='one frame less, frames = len')
    assert got[0][0] == -np.inf


def test_ragged_batch_reads_no_padding():
    rng = np.random.default_rng(4)
    frames, ld = 37, 12
    lengths, target_lengths = [0, 37, 20, 0, 9], [3, 0, 7, 0, 4]
    lp = _log_probs(rng, 5, frames)
    targets = np.full((5, ld), 999, np.int32)
    for b in range(5):
        lp[b, lengths[b]:] = np.nan
        targets[b, :target_lengths[b]] = _labels(rng, target_lengths[b])
    got = _check(lp, lengths, targets, target_lengths, what='ragged')
    assert got[0][0] == -np.inf and got[0][3] == 0 and np.isfinite(got[0][[1, 2, 4]]).all()
    assert (got[1][1] == 0).all()                                  # no labels: the path is all blank
    # lengths beyond the tensors are clamped: len > frames and L > ld_targets read what frames and ld_targets allow
    targets = np.stack([_labels(rng, ld) for _ in range(5)])
    lp = _log_probs(rng, 5, frames)
    _assert_bits(_device(lp, [99, 37, -4, 40, 37], targets, [12, 50, 3, -1, 12]), _device(lp, [37, 37, 0, 37, 37], targets, [12, 12, 3, 0, 12]), 'clamped')


def test_ties_follow_the_rule():
    """Log-probs from {0, -0.5, -1, -1.5}: every sum is exact in fp32 and equal maxima are common; 3 classes and labels of two values, so that
    skips are often forbidden.  The path must be the tie rule's: the model's, bit for bit."""
    rng = np.random.default_rng(5)
    b, frames, ld = 24, 24, 8
    lp = (-0.5 * rng.integers(0, 4, size=(b, frames, 3))).astype(np.float32)
    targets = rng.integers(1, 3, size=(b, ld)).astype(np.int32)
    lengths = rng.integers(10, frames + 1, size=b)
    target_lengths = rng.integers(0, ld + 1, size=b)
    got = _check(lp, lengths, targets, target_lengths, what='ties')
    assert np.isfinite(got[0]).sum() >= b // 2
    zeros = _check(np.zeros((2, 9, 3), np.float32), [9, 9], np.array([[1, 2, 1], [1, 1, 2]], np.int32), [3, 3], what='all equal')
    assert zeros[1][0].tolist() == [1, 2, 1, 1, 1, 1, 1, 1, 1] and zeros[1][1].tolist() == [1, 0, 1, 2, 2, 2, 2, 2, 2]


def test_other_blank_masked_class_and_bad_labels():
    rng = np.random.default_rng(6)
    lp = _log_probs(rng, 3, 30)
    targets = np.stack([_labels(rng, 9, blank=2) for _ in range(3)])
    got = _check(lp, [30, 25, 30], targets, [9, 5, 0], blank=2, what='blank = 2')
    assert np.isfinite(got[0]).all() and (got[1][2] == 2).all()
    # class 7 masked everywhere: a transcript without it aligns as usual, one with it has no path
    lp = _log_probs(rng, 2, 30)
    lp[:, :, 7] = -np.inf
    targets = np.stack([_labels(rng, 9, blank=7), _labels(rng, 9, blank=7)])
    targets[targets == 0] = 1
    targets[1, 4] = 7
    got = _check(lp, [30, 30], targets, [9, 9], what='masked class')
    assert np.isfinite(got[0][0]) and got[0][1] == -np.inf
    # a label equal to the blank, a label equal to `classes`: NaN for that utterance only; the same labels beyond L are never read
    lp = _log_probs(rng, 5, 30)
    targets = np.stack([_labels(rng, 9) for _ in range(5)])
    clean = _device(lp, [30] * 5, targets, [9, 9, 9, 6, 6])
    targets[1, 3], targets[2, 8], targets[3, 7], targets[4, 6] = 0, CLASSES, 0, CLASSES
    got = _check(lp, [30] * 5, targets, [9, 9, 9, 6, 6], what='bad labels')
    assert np.isnan(got[0][[1, 2]]).all() and np.isfinite(got[0][[0, 3, 4]]).all()
    for b in (0, 3, 4):
        for g, c in zip(got, clean):
            assert np.array_equal(g[b].view(np.int32), c[b].view(np.int32)), b
    _check(lp, [30] * 5, np.where(targets == CLASSES, -1, targets).astype(np.int32), [9, 9, 9, 6, 6], what='negative label')


def test_repeatable_and_on_any_stream():
    rng = np.random.default_rng(8)
    lp = torch.from_numpy(_log_probs(rng, 6, 80)).to(DEV)
    targets = torch.from_numpy(np.stack([_labels(rng, 20) for _ in range(6)])).to(DEV)
    lengths, target_lengths = [80, 70, 60, 50, 45, 80], [20, 18, 5, 20, 20, 0]
    first = ctc.forced_align(lp, lengths, targets, target_lengths)
    second = ctc.forced_align(lp, lengths, targets, target_lengths)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        third = ctc.forced_align(lp, lengths, targets, target_lengths)
    side.synchronize()
    torch.cuda.current_stream(DEV).wait_stream(side)
    assert isinstance(first, ctc.Alignment) and first._fields == ('path', 'score', 'starts', 'ends', 'token_scores')
    for a, b, c in zip(first, second, third):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(a.view(torch.int32), c.view(torch.int32))


def test_forced_align_refuses_what_it_cannot_take():
    lp = torch.zeros(2, 6, 5, device=DEV)
    targets = torch.ones(2, 2, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match='float32 on a HIP device'):
        ctc.forced_align(lp.double(), [6, 6], targets, [2, 2])
    with pytest.raises(ValueError, match='no CPU path'):
        ctc.forced_align(lp.cpu(), [6, 6], targets, [2, 2])
    with pytest.raises(ValueError, match=r'targets must be \(2, labels\)'):
        ctc.forced_align(lp, [6, 6], targets[0], [2, 2])
    with pytest.raises(ValueError, match=r'log_probs must be \(batch, frames, classes\)'):
        ctc.forced_align(lp[0], [6, 6], targets, [2, 2])
    with pytest.raises(ValueError, match='expected 2 lengths'):
        ctc.forced_align(lp, [6], targets, [2, 2])
    with pytest.raises(nb.hip.HipError, match='blank=5'):
        ctc.forced_align(lp, [6, 6], targets, [2, 2], blank=5)


def test_align_runs_the_model_and_aligns_its_output():
    m = nb.get_model([[1, 0], [1, 0, 0], [1, 0, 0, 0]], use_rnn=True, dropout_rate=0.0)
    keyed_fill_(m, seed=1235, mode='lively')
    m = m.to(DEV).train()
    x = keyed_input(2, 64, seed=3).to(DEV)
    targets = torch.tensor([[5, 5, 17], [40, 2, 9]], dtype=torch.int32)
    audio_len, targets_len = torch.tensor([64, 50]), torch.tensor([3, 2])
    got = ctc.align(m, x, audio_len, targets, targets_len)
    assert m.training and not any(t.requires_grad for t in got)                 # the eval() forward, no gradients, the flag put back
    m.eval()
    with torch.no_grad():
        lp = ctc.log_softmax(m(x))
    want = ctc.forced_align(lp, [16, 12], targets.to(DEV), targets_len)
    assert got.path.shape == (2, 16) and torch.isfinite(got.score).all()
    for g, w in zip(got, want):
        assert torch.equal(g.view(torch.int32), w.view(torch.int32))
    _assert_bits(tuple(t.cpu().numpy() for t in (got.score, got.path, got.starts, got.ends, got.token_scores)),
                 model.align_batch(lp.cpu().numpy(), [16, 12], targets.numpy(), [3, 2], 0, np.float32), 'model output')
    assert ctc.FRAME_SECONDS == pytest.approx(0.04) and ctc.FRAME_SECONDS == 4 * 160 / 16000
