"""Plain-Python model of the prefix beam search AS THE KERNEL DEFINES IT, with per-token time steps and bigram LM fusion (helper of
test_beam_timesteps_host.py, test_beam_timesteps_gpu.py, test_beam_lm_host.py and test_beam_lm_gpu.py; no tests here).

Not a trie: a list of live prefixes (what the lanes of ``beam_frame`` hold) plus a list of token nodes ``[parent, class, frame, best]``
(the pool).  Prefix identity is the token string (the kernel's 64-bit hash), candidates are ordered like ``beam_key`` (score descending,
last class ascending, slot ascending), and the arithmetic is numpy float32 in the order of ``oracle.decode_oracle.log_sum_exp`` -- so
tokens and scores equal the oracle's (test_beam_timesteps_host.py anchors that first).  The time steps follow DESIGN.md §9 "Beam decode":

1. creation: a new prefix (live prefix + class c, not itself live) that survives frame t gets a node with the record (t, lp_t[c]);
2. update: a prefix live on entry to frame t whose string minus its last token is live too, last class c: if c survived the pruning
   and lp_t[c] > best (strictly), its OWN node's record becomes (t, lp_t[c]) -- whether or not the parent contributes probability;
3. re-creation: a prefix that dropped out and is spelled again gets a new node with a fresh record; beams built on the old node keep it;
4. t is the utterance's own 0-based frame index.

``fusion`` is the table W of include/nbasr.h "bigram LM fusion", one line per rule of its contract (marked below).  Staying on blank and
repeating the last class get nothing, -FLT_MAX stays -FLT_MAX, and the time-step records look at ``lp`` only.

``dtype=np.float64`` accumulates the scores in float64 (same inputs): the tests use seeds at which that changes no beam, so a device whose
exp / log differ in the last bit is not expected to break a tie differently.
"""
import numpy as np
import torch

NEG = -np.finfo(np.float32).max
LANES = 64                                    # BEAM_CLASSES of the kernel: the slot of a candidate is source * LANES + class


def _lse(x, y, F):
    if x <= NEG:
        return y
    if y <= NEG:
        return x
    m = max(x, y)
    return F(F(np.log(F(np.exp(F(x - m))) + F(np.exp(F(y - m))))) + m)


class _Live:
    __slots__ = ('b', 'nb', 'score', 'last', 'node', 'tokens')

    def __init__(self, b, nb, score, last, node, tokens):
        self.b, self.nb, self.score, self.last, self.node, self.tokens = b, nb, score, last, node, tokens


def beam_search(log_probs, beam_width=12, blank=0, cutoff_top_n=40, dtype=np.float32, stats=None, fusion=None):
    """log_probs (T, C) float32 of ONE utterance -> [(tokens, -score, timesteps)], best first, at most ``beam_width`` entries.
    ``stats`` (dict): counts 'updates' (rule 2 moved a record) and 'recreated_under_live' (rule 3: a prefix got a second node while a
    live prefix was still built on its first one).  ``fusion``: the table W, (classes, classes) float32, of the fused search."""
    F = dtype
    W = None if fusion is None else np.asarray(fusion, dtype=np.float32)
    lp_all = np.asarray(log_probs, dtype=np.float32)
    n_cls = lp_all.shape[1] if lp_all.ndim == 2 else 0
    nodes = [[-1, -1, 0, NEG]]                                     # the root
    live = [_Live(F(0.0), F(NEG), F(0.0), -1, 0, ())]
    had_node = {}                                                  # token string -> its latest node
    if stats is not None:
        stats.setdefault('updates', 0)
        stats.setdefault('recreated_under_live', 0)
    for t in range(lp_all.shape[0]):
        row = lp_all[t]
        order = sorted(range(n_cls), key=lambda c: (-float(row[c]), c))
        kept = set(order[:cutoff_top_n] if cutoff_top_n < n_cls else order)
        lp = [F(row[c]) if c in kept and row[c] > NEG else F(NEG) for c in range(n_cls)]
        index = {p.tokens: j for j, p in enumerate(live)}
        cands = []                                                 # (score, last + 1, slot, source, class or None)
        stay = []
        for j, p in enumerate(live):
            mp = index.get(p.tokens[:-1]) if p.tokens else None
            lp_last = lp[p.last] if p.last >= 0 else F(NEG)
            if mp is not None and lp_last > NEG and lp_last > nodes[p.node][3]:         # rule 2
                nodes[p.node][2], nodes[p.node][3] = t, lp_last
                if stats is not None:
                    stats['updates'] += 1
            n_b = F(lp[blank] + p.score) if lp[blank] > NEG else F(NEG)
            n_nb = F(NEG)
            if p.last >= 0 and lp_last > NEG:
                n_nb = F(lp_last + p.nb)
                if mp is not None:
                    par = live[mp]
                    if p.last == par.last:
                        add = F(lp_last + par.b) if par.b > NEG else F(NEG)
                    else:
                        add = F(lp_last + par.score)
                    if W is not None and add > NEG:                # fusion: the mass a live prefix absorbs from its live parent
                        add = F(add + F(W[par.last if par.last >= 0 else blank][p.last]))
                    n_nb = _lse(n_nb, add, F)
            n_score = _lse(n_b, n_nb, F)
            stay.append((n_b, n_nb, n_score))
            cands.append((n_score, p.last + 1, beam_width * LANES + j, j, None))
        for i, p in enumerate(live):
            for c in range(n_cls):
                if c == blank or not lp[c] > NEG or p.tokens + (c,) in index:
                    continue
                if c == p.last:
                    v = F(lp[c] + p.b) if p.b > NEG else F(NEG)
                else:
                    v = F(lp[c] + p.score)
                if W is not None and v > NEG:                      # fusion: a candidate, live prefix p + class c
                    v = F(v + F(W[p.last if p.last >= 0 else blank][c]))
                cands.append((v, c + 1, i * LANES + c, i, c))
        cands.sort(key=lambda k: (-float(k[0]), k[1], k[2]))
        nxt = []
        for v, _, _, src, c in cands[:beam_width]:
            p = live[src]
            if c is None:
                n_b, n_nb, n_score = stay[src]
                nxt.append(_Live(n_b, n_nb, n_score, p.last, p.node, p.tokens))
            else:
                nodes.append([p.node, c, t, lp[c]])                # rule 1 (and 3: always a new node)
                nxt.append(_Live(F(NEG), v, v, c, len(nodes) - 1, p.tokens + (c,)))
        if stats is not None:
            for q in nxt:
                old = had_node.get(q.tokens)
                if old is not None and old != q.node and any(_on_chain(nodes, o.node, old) for o in nxt if o is not q):
                    stats['recreated_under_live'] += 1
        for q in nxt:
            had_node[q.tokens] = q.node
        live = nxt
    out = []
    for p in live:
        steps, node = [], p.node
        while node > 0:
            steps.append(nodes[node][2])
            node = nodes[node][0]
        out.append((list(p.tokens), -float(p.score), steps[::-1]))
    return out


def _on_chain(nodes, node, target):
    while node > 0:
        if node == target:
            return True
        node = nodes[node][0]
    return False


# ---- the cases both test files use -------------------------------------------------------------------------------------------------

def log_probs(shape, seed, sharp=2.0):
    gen = torch.Generator().manual_seed(seed)
    return torch.log_softmax(torch.randn(*shape, generator=gen) * sharp, dim=-1)


# (b, frames, classes, width, top_n, sharp) of test_decode.py::test_gpu_beam_search_matches_oracle: all of them anchor the model, the
# timed search is tested at TIMED_SHAPES.  With that test's seeds (and the narrow-beam sweep's) the float32 and the float64 model return
# the same beams everywhere (test_beam_timesteps_host.py asserts it), so no seed had to be moved.
ORACLE_SHAPES = [(3, 40, 49, 12, 40, 2.0), (2, 60, 49, 12, 40, 0.5), (2, 25, 5, 4, 40, 1.0), (2, 30, 49, 1, 40, 3.0), (1, 20, 49, 32, 40, 1.0),
                 (2, 12, 3, 12, 40, 1.0), (1, 30, 64, 8, 10, 1.0), (2, 1, 49, 12, 40, 1.0), (1, 16, 2, 3, 1, 1.0)]
TIMED_SHAPES = [(3, 40, 49, 12, 40, 2.0), (2, 25, 5, 4, 40, 1.0), (2, 30, 49, 1, 40, 3.0), (1, 30, 64, 8, 10, 1.0), (2, 1, 49, 12, 40, 1.0),
                (1, 16, 2, 3, 1, 1.0)]


def fusion_table(classes, seed_offset=5):
    """The table of the tie-freedom test and of the device comparison: W = (default_rng(5 + C).normal(size=(C, C)) - 0.5) in float32."""
    return (np.random.default_rng(seed_offset + classes).normal(size=(classes, classes)) - 0.5).astype(np.float32)


def shape_input(shape):
    """Log-probabilities of a shape the way test_gpu_beam_search_matches_oracle builds them (blanks win often)."""
    b, frames, classes, width, top_n, sharp = shape
    lp = log_probs((b, frames, classes), 100 * frames + classes + width, sharp)
    lp[:, ::3, 0] += 1.5
    return torch.log_softmax(lp, dim=2)


def narrow_cases():
    """The 40 cases of test_gpu_beam_search_narrow_beams_sweep: [(width, classes, frames, log_probs (2, frames, classes))]."""
    rng = np.random.default_rng(7)
    cases = []
    for case in range(40):
        width, classes, frames = int(rng.integers(2, 5)), int(rng.integers(3, 6)), int(rng.integers(20, 61))
        sharp = float(rng.choice([0.3, 1.0, 2.0]))
        cases.append((width, classes, frames, log_probs((2, frames, classes), 1000 + case, sharp)))
    return cases


def lengths_of(b, frames):
    return [frames, frames // 2, 0][:b]


def utterances(shape):
    """[(key, log_probs (n, classes) numpy, width, top_n)] of a shape: every utterance whole, then cut to the ragged lengths."""
    b, frames, _, width, top_n, _ = shape
    lp = shape_input(shape).numpy()
    out = [((shape, 'whole', i), lp[i], width, top_n) for i in range(b)]
    return out + [((shape, 'ragged', i), lp[i, :n], width, top_n) for i, n in enumerate(lengths_of(b, frames))]


def narrow_utterances():
    return [(('narrow', k, i), lp[i].numpy(), width, 40) for k, (width, _, _, lp) in enumerate(narrow_cases()) for i in range(2)]


def peaked(b, frames, classes=49, seed=11):
    """Peaked log-probabilities (one class near probability 1 per frame, a blank every other frame) and the argmax path (b, frames)."""
    gen = torch.Generator().manual_seed(seed)
    path = torch.randint(1, classes, (b, frames), generator=gen)
    path[:, ::2] = 0
    path[:, 5:9] = path[:, 5:6]                                   # a run of one class: a repeat, not a new token
    path[:, 12] = path[:, 11]
    logits = torch.randn(b, frames, classes, generator=gen)
    logits.scatter_(2, path.unsqueeze(2), 12.0)
    return torch.log_softmax(logits, dim=2), path


def argmax_run_starts(path, blank=0):
    """(tokens, first frames) of the argmax runs of a path, blanks dropped: greedy CTC with the frame each token starts at."""
    tokens, starts = [], []
    for t, c in enumerate(path):
        if c != blank and (t == 0 or c != path[t - 1]):
            tokens.append(int(c))
            starts.append(t)
    return tokens, starts


def same_beams(a, b):
    return [tok for tok, _, _ in a] == [tok for tok, _, _ in b]


def _pruned(lp, top_n):
    """(frames, classes) bool: the class took no part in the frame (the kernel's pre-pass: rank >= top_n, ties to the lower class)."""
    order = np.argsort(-lp, axis=1, kind='stable')
    rank = np.empty_like(order)
    np.put_along_axis(rank, order, np.arange(lp.shape[1])[None, :], axis=1)
    return rank >= top_n


def check_timestep_properties(key, lp, width, top_n, beams):
    """beams: [(tokens, score, timesteps)].  Token k of a beam cannot exist before frame k, its frame is one of the utterance's, and its class
    took part in that frame; width 1 never has a parent live beside its child, so every step is a creation and the sequence increases."""
    pruned = _pruned(lp, top_n) if len(lp) else None
    for r, (tok, _, steps) in enumerate(beams):
        assert len(steps) == len(tok), (key, r)
        for k, (c, ts) in enumerate(zip(tok, steps)):
            assert k <= ts < len(lp), (key, r, k, ts)
            assert not pruned[ts, c], (key, r, k, ts, c)
        if width == 1:
            assert all(a < b for a, b in zip(steps, steps[1:])), (key, r, steps)
