"""Exactly summable operands for one grouped-convolution cell, their fp64 reference, and the cases the GPU file runs them at.

The grouped-conv kernels are compared elsewhere through tolerances that the order of their sums and the rounding of their results
force.  On the operands built here every product and every partial sum is a small integer: exact in bfloat16 and in float32 whatever
the order, so every kernel of the family must equal the fp64 evaluation AS NUMBERS, element by element, and a single wrong index, tap,
pad, skip or group is a different integer.  ``tests/test_cell_exact_host.py`` asserts -- without a GPU -- the conditions that keep this
net from going blind (CONDITIONS below) for every case ``tests/test_cell_exact_gpu.py`` runs.

Plain CPU code: torch, the oracle and the keyed generator; nothing here imports the HIP bindings.
"""
import collections
import functools

import numpy as np
import torch
import torch.nn.functional as F

from nb_asr_amd.utils import keyed_uniform
from oracle import asr_oracle as oracle

# one cell: channels per group, groups, frames, three (taps, dilation), skip mask (bit0 s00 | bit1 s10 | bit2 s11 | bit3 s20 | bit4 s21 |
# bit5 s22), pending LayerNorm on the cell input, utterances
Case = collections.namedtuple('Case', 'cg groups t kds mask with_ln batch')
Operands = collections.namedtuple('Operands', 'x0 ln nodes')                   # ln: (mean, rstd, gamma, beta) or None; nodes: 3 x (w, bias, k, d)
Reference = collections.namedtuple('Reference', 'x0n x1 x2 x3 pre')           # fp64; pre: the three pre-activation tensors

NONZEROS = (6, 4, 3)            # nonzero weights per output channel of nodes 0 / 1 / 2: the later the node, the larger its input
MAX_ABS = 256                   # integers up to 2^8 are exact in bfloat16 (8 significand bits)
LIVE_SHARE = 0.2                # of a node's pre-activations strictly inside (0, CLAMP): relu and the clamp erase an error outside
SEED = 1

# the (kds, mask, with_ln) combinations every shape runs, and one each with every skip and with none
COMBO_LN = (((7, 2), (5, 1), (7, 2)), 0b101001, True)
COMBO_PLAIN = (((5, 2), (7, 2), (7, 1)), 0b010110, False)
COMBO_ALL = (((7, 1), (7, 2), (5, 2)), 63, True)
COMBO_NONE = (((5, 1), (5, 1), (5, 1)), 0, True)
COMBOS = (COMBO_LN, COMBO_PLAIN)

CGS = (6, 8, 10, 12)
GROUPS, BATCH = 4, 2


# ---- operands ----------------------------------------------------------------------------------------------------------------------
def _ints(key, shape, lo, hi, seed=SEED):
    """Keyed integers uniform in [lo, hi], as float64."""
    u = keyed_uniform(key, seed, shape, 0.0, 1.0).astype(np.float64)
    return torch.from_numpy(np.minimum(np.floor(u * (hi - lo + 1)), hi - lo) + lo)


def _choice(key, shape, values, seed=SEED):
    return torch.tensor(values, dtype=torch.float64)[_ints(key, shape, 0, len(values) - 1, seed).long()]


def _weights(key, groups, cg, k, nonzeros, seed=SEED):
    """(groups * cg, cg, k) weights in {-1, 0, 1}, `nonzeros` per output channel.  The positions are dealt from keyed shuffles of the
    cg * k (input channel, tap) pairs, one shuffle after the other over the output channels of ALL groups: the first shuffle is dealt out
    whole, so every (input channel, tap) carries a weight in some group (condition c)."""
    c, p = groups * cg, cg * k
    assert c * nonzeros >= p, 'too few nonzeros to cover every (input channel, tap)'
    n_shuffles = -(-c * nonzeros // p)
    order = np.concatenate([np.argsort(keyed_uniform(f'{key}/shuffle{i}', seed, (p,), 0.0, 1.0), kind='stable') for i in range(n_shuffles)])
    sign = _choice(f'{key}/sign', (c, nonzeros), (-1.0, 1.0), seed)
    w = torch.zeros(c, p, dtype=torch.float64)
    for co in range(c):
        taken = []
        for pos in order[co * nonzeros:(co + 1) * nonzeros]:
            pos = int(pos)
            while pos in taken:                       # (across the seam of two shuffles a position can come twice: take the next free one)
                pos = (pos + 1) % p
            taken.append(pos)
        for j, pos in enumerate(taken):
            w[co, pos] = sign[co, j]
    return w.view(c, cg, k)


@functools.lru_cache(maxsize=None)
def operands(case):
    """x0 integers in [-2, 2]; the pending LayerNorm as given statistics (mean in {-1, 0, 1}, rstd in {1, 2} per frame) and parameters
    (gamma in {-1, 1}, beta in {-1, 0, 1} per channel); weights in {-1, 0, 1}; biases integers in [0, 3].  float64 tensors holding
    bf16-representable values: the same operands serve both storage types."""
    c = case.cg * case.groups
    key = f'cell_exact/cg{case.cg}g{case.groups}t{case.t}m{case.mask}/' + ''.join(f'{k}{d}' for k, d in case.kds)
    x0 = _ints(key + '/x0', (case.batch, c, case.t), -2, 2)
    ln = None
    if case.with_ln:
        ln = (_ints(key + '/mean', (case.batch, case.t), -1, 1), _ints(key + '/rstd', (case.batch, case.t), 1, 2),
              _choice(key + '/gamma', (c,), (-1.0, 1.0)), _ints(key + '/beta', (c,), -1, 1))
    nodes = tuple((_weights(f'{key}/w{i}', case.groups, case.cg, k, NONZEROS[i]), _ints(f'{key}/b{i}', (c,), 0, 3), k, d)
                  for i, (k, d) in enumerate(case.kds))
    return Operands(x0, ln, nodes)


# ---- reference ---------------------------------------------------------------------------------------------------------------------
def normalised(x0, ln):
    if ln is None:
        return x0
    mean, rstd, gamma, beta = ln
    return (x0 - mean[:, None, :]) * rstd[:, None, :] * gamma[None, :, None] + beta[None, :, None]


def pre_activation(x, w, bias, dilation, groups):
    """The convolution of ``oracle.pad_conv_relu`` before its relu and clamp, with the oracle's padding."""
    lpad, rpad = oracle.pad_amounts(w.shape[-1], dilation, 1)
    return F.conv1d(F.pad(x, (lpad, rpad)), w, bias, dilation=dilation, groups=groups)


def evaluate(ops, case):
    """The reference's cell in fp64: PadConvRelu (clamp at 20) per node, then the skips in python's sum order (cell input, x1, x2)."""
    s = [bool(case.mask >> i & 1) for i in range(6)]
    flags = ((s[0],), (s[1], s[2]), (s[3], s[4], s[5]))
    outs, pre = [normalised(ops.x0, ops.ln)], []
    for (w, bias, _, d), node_flags in zip(ops.nodes, flags):
        out = oracle.pad_conv_relu(outs[-1], w, bias, d, 1, case.groups)
        pre.append(pre_activation(outs[-1], w, bias, d, case.groups))
        for flag, src in zip(node_flags, outs):
            if flag:
                out = out + src
        outs.append(out)
    return Reference(*outs, tuple(pre))


@functools.lru_cache(maxsize=None)
def reference(case):
    """Cached per case: it depends on no tiling, pitch or storage type.  Do not modify what it returns."""
    return evaluate(operands(case), case)


# ---- CONDITIONS that keep the comparison from going blind (asserted on the reference alone) -------------------------------------------
def check_conditions(case):
    ops, ref = operands(case), reference(case)
    # (a) every tensor integer-valued with magnitude <= 256: exact in bf16 and fp32 whatever the order of the sums
    tensors = {'x0': ops.x0, 'x0n': ref.x0n, 'x1': ref.x1, 'x2': ref.x2, 'x3': ref.x3, 'pre0': ref.pre[0], 'pre1': ref.pre[1], 'pre2': ref.pre[2]}
    for name, v in tensors.items():
        assert v.dtype == torch.float64 and bool((v == v.round()).all()), (case, name, 'not integer-valued')
        assert float(v.abs().max()) <= MAX_ABS, (case, name, float(v.abs().max()))
    # ... and so is every partial sum: the sum of the magnitudes of a pre-activation's terms bounds each of them
    for i, (w, bias, _, d) in enumerate(ops.nodes):
        src = (ref.x0n, ref.x1, ref.x2)[i]
        assert float(pre_activation(src.abs(), w.abs(), bias.abs(), d, case.groups).max()) <= MAX_ABS, (case, i, 'a partial sum may exceed 256')
    # (b) at least LIVE_SHARE of every node's pre-activations strictly inside (0, 20)
    shares = [float(((p > 0) & (p < oracle.CLAMP)).double().mean()) for p in ref.pre]
    assert min(shares) >= LIVE_SHARE, (case, shares)
    # (c) over the groups, every (input channel, tap) of every node carries a nonzero weight
    for i, (w, _, k, _) in enumerate(ops.nodes):
        used = (w.view(case.groups, case.cg, case.cg, k) != 0).any(dim=1).any(dim=0)            # [input channel][tap]
        assert bool(used.all()), (case, i, 'an (input channel, tap) without a weight')
    for i, (w, _, _, _) in enumerate(ops.nodes):
        assert bool(((w != 0).sum(dim=(1, 2)) == NONZEROS[i]).all()), (case, i)
    return shares


def statistics(x, eps=oracle.LN_EPS):
    """fp64 (mean, 1 / sqrt(var + eps)) over the channels of x (B, C, T)."""
    return x.mean(dim=1), 1.0 / torch.sqrt(x.var(dim=1, unbiased=False) + eps)


# ---- the cases of the GPU file ---------------------------------------------------------------------------------------------------------
def mfma_nbts(cg):
    """The 16-frame blocks per wave that ``NBASR_CELLM_TILING`` can force: the 16-slot groups (10, 12 channels) have two instantiations."""
    return (8, 10, 14, 16) if cg <= 8 else (8, 16)


def mfma_frames(nbt):
    """Frame counts for wave tiles of W = 16 nbt frames: the 8-frame global chunk and the 16-frame block; the partner column block of the
    8-slot form (W / 2 apart); the row end at a wave-tile seam; a last tile of fifteen frames; three waves."""
    w = 16 * nbt
    return (1, 7, 8, 9, w // 2 - 1, w // 2 + 1, w - 1, w, w + 1, w + 15, 2 * w + 1)


MFMA_GPWS = (1, 2, 4)
VECTOR_FRAMES = (1, 3, 4, 5, 255, 256, 257, 513)           # the 4-frame lane chunk and the 256-frame wave of grouped_cell.hip
PLANNER_FRAMES = 150                                       # two wave tiles of the tiling the planner takes for it, the seam inside the row
SENSITIVITY = Case(8, GROUPS, 137, *COMBO_LN, BATCH)


def case(cg, t, combo, groups=GROUPS):
    return Case(cg, groups, t, *combo, BATCH)


def mfma_forced_cases():
    """(cg, nbt, t): every one runs COMBOS at every groups-per-workgroup of MFMA_GPWS."""
    return [(cg, nbt, t) for cg in CGS for nbt in mfma_nbts(cg) for t in mfma_frames(nbt)]


def mfma_wide_pitch_cases():
    """(cg, nbt, t): rows whose pitch is a whole wave tile larger than they need -- a tile wholly past the row end."""
    return [(cg, nbt, 16 * nbt + 1) for cg in CGS for nbt in mfma_nbts(cg)]


def mfma_other_cases():
    """Every skip and none at a wave-tile seam of the smallest tile, and 5 / 6 groups on the planner's own tiling."""
    return ([case(cg, 129, combo) for cg in CGS for combo in (COMBO_ALL, COMBO_NONE)]
            + [case(cg, PLANNER_FRAMES, COMBO_LN, groups) for cg in CGS for groups in (5, 6)])


def vector_cases():
    return [case(cg, t, combo) for cg in CGS for t in VECTOR_FRAMES for combo in COMBOS] + [case(cg, 257, combo) for cg in CGS for combo in (COMBO_ALL, COMBO_NONE)]


def all_cases():
    seen = {case(cg, t, combo) for cg, _, t in mfma_forced_cases() + mfma_wide_pitch_cases() for combo in COMBOS}
    return sorted(seen | set(mfma_other_cases()) | set(vector_cases()) | {SENSITIVITY})


# ---- the sensitivity probe -----------------------------------------------------------------------------------------------------------
def move_one_tap(ops, node=2):
    """A copy of the operands in which ONE nonzero weight of `node` sits on the neighbouring tap: (operands, (co, ci, tap, new tap))."""
    w = ops.nodes[node][0].clone()
    k = w.shape[-1]
    for co, ci, tap in (w != 0).nonzero().tolist():
        new = tap + 1 if tap + 1 < k else tap - 1
        if w[co, ci, new] == 0:
            w[co, ci, new], w[co, ci, tap] = w[co, ci, tap].item(), 0.0
            nodes = list(ops.nodes)
            nodes[node] = (w,) + ops.nodes[node][1:]
            return Operands(ops.x0, ops.ln, tuple(nodes)), (co, ci, tap, new)
    raise AssertionError('no weight with a free neighbouring tap')
