"""Plain-Python model of the prefix beam search with bigram LM fusion AS THE KERNEL DEFINES IT (helper of test_beam_lm_host.py and
test_beam_lm_gpu.py; no tests here).

The search of beam_timesteps_model.py (imported for its shapes and inputs) with ``fusion=None`` added: ``fusion`` is the table W of
include/nbasr.h "bigram LM fusion", (classes, classes) float32.  Two lines differ from that model, one per rule of the contract:

1. a candidate (live prefix p + class c): after ``v`` is formed, ``if v > NEG: v = F(v + F(W[p.last or blank][c]))``;
2. the mass a live prefix absorbs from its live parent: after ``add`` is formed, ``if add > NEG: add = F(add + F(W[par.last or blank][p.last]))``.

Staying on blank and repeating the last class get nothing, -FLT_MAX stays -FLT_MAX, and the time-step records look at ``lp`` only.
"""
import numpy as np

from beam_timesteps_model import LANES, NEG, _Live, _lse


def fusion_table(classes, seed_offset=5):
    """The table of the tie-freedom test and of the device comparison: W = (default_rng(5 + C).normal(size=(C, C)) - 0.5) in float32."""
    return (np.random.default_rng(seed_offset + classes).normal(size=(classes, classes)) - 0.5).astype(np.float32)


def beam_search(log_probs, beam_width=12, blank=0, cutoff_top_n=40, dtype=np.float32, fusion=None):
    """log_probs (T, C) float32 of ONE utterance -> [(tokens, -score, timesteps)], best first, at most ``beam_width`` entries."""
    F = dtype
    W = None if fusion is None else np.asarray(fusion, dtype=np.float32)
    lp_all = np.asarray(log_probs, dtype=np.float32)
    n_cls = lp_all.shape[1] if lp_all.ndim == 2 else 0
    nodes = [[-1, -1, 0, NEG]]                                     # the root
    live = [_Live(F(0.0), F(NEG), F(0.0), -1, 0, ())]
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
            if mp is not None and lp_last > NEG and lp_last > nodes[p.node][3]:
                nodes[p.node][2], nodes[p.node][3] = t, lp_last
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
                    if W is not None and add > NEG:
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
                if W is not None and v > NEG:
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
                nodes.append([p.node, c, t, lp[c]])
                nxt.append(_Live(F(NEG), v, v, c, len(nodes) - 1, p.tokens + (c,)))
        live = nxt
    out = []
    for p in live:
        steps, node = [], p.node
        while node > 0:
            steps.append(nodes[node][2])
            node = nodes[node][0]
        out.append((list(p.tokens), -float(p.score), steps[::-1]))
    return out
